"""Host-side mirror of the reference's detection-op interfaces, bound to libminddet_hip.so.

Names, argument meaning and return conventions follow the reference so that its call sites
read the same (paths relative to /root/reference/minddet/models):

  NMS                     centerpoint/det3d_ms/ops/nms_cpu.py:7-27     (boxes[N,7], thresh) -> (keep[N] i32, num)
  BoxesIouBevGpu, BoxesOverlapBevGpu, NumGpu, NmsNormalGpu
                          centerpoint/det3d_ms/ops/test_custom_pytorch/iou_gpu.py:14-81
  boxes_iou_bev, boxes_iou3d_gpu, nms_gpu, nms_normal_gpu
                          centerpoint/det3d_ms/ops/iou3d_nms/iou3d_nms_utils.py:12-116
  iou_jit                 pointpillars/src/core/box_np_ops.py:639-679
  nms_jit / apply_nms     pointpillars/src/core/nms.py:7-41,85-112     (via nms_aligned)
  circle_nms              centerpoint/det3d_ms/core/utils/circle_nms_jit.py:6-36
  cp_assign_targets, CenterPointTargets
                          centerpoint/det3d_ms/datasets/pipelines/preprocess.py:285-521 (AssignLabel, for a batch)
  cp_loss, CenterPointLoss, center_point_loss
                          centerpoint/det3d_ms/models/bbox_heads/center_head.py:208-271 (CenterHead.loss) with
                          centerpoint/det3d_ms/models/losses/centernet_loss.py:22-82 (FastFocalLoss, RegLoss)
  pp_loss, PointPillarsLoss, point_pillars_loss
                          pointpillars/src/pointpillars.py:817-872 (PointPillarsWithLossCell.construct behind the network) with
                          pointpillars/src/core/losses.py:40-191; assign_targets_batch stacks assign_targets per sample
  cn_assign_targets, CenterNetTargets
                          centernet/src/dataset.py:317-384 (the target part of COCOHP.preprocess_fn, for a batch) with
                          centernet/src/image.py:59-63,94-144
  cn_loss, CenterNetLoss, center_net_loss
                          centernet/src/centernet_det.py:177-237 (CenterNetLossCell.construct behind the network) with
                          centernet/src/utils.py:132-245 (Sigmoid, FocalLoss, RegLoss)
  cn_aug_transform, cn_aug_image, CenterNetAugment
                          centernet/src/dataset.py:278-315 (the training branch of COCOHP.preprocess_fn in front of the targets)
                          with centernet/src/image.py:25-57,208-253 (get_affine_transform, color_aug)
  KittiCalibration, crop_hulls, kitti_boxes_to_lidar, kitti_rows
                          pointpillars/src/core/box_np_ops.py:395-449, 581-636 (remove_outside_points, the frustums, box_camera_to_lidar),
                          pointpillars/src/data/preprocess.py:59-71, 87 and pointpillars/src/predict.py:204-262, 331-396
  kitti_eval_flags, kitti_eval_overlaps, kitti_eval_match, kitti_eval_thresholds, kitti_eval_stats
                          pointpillars/eval_gpu/eval.py:9-297, 483-599 (clean_data, the three overlaps, compute_statistics,
                          get_thresholds and the sums of eval_class, for all images at once; minddet_amd/kitti_eval.py drives them)
  coco_eval_rows, coco_eval_match, coco_eval_accumulate
                          centernet/src/post_process.py:64-89 (to_float, convert_eval_format) and the COCOeval bbox evaluate() /
                          accumulate() called at centernet/eval.py:181-187; minddet_amd/coco_eval.py drives them
  nusc_rows, nusc_eval_match, nusc_eval_accumulate
                          centerpoint/det3d_ms/datasets/nuscenes/nusc_common.py:160-201 (_second_det_to_nusc_box,
                          _lidar_nusc_box_to_global), nuscenes.py:252-293 (the attribute rule) and the devkit's DetectionEval called at
                          nusc_common.py:659-674; minddet_amd/nusc_eval.py drives them

All tensors are torch CUDA tensors; work is enqueued on the current stream; nothing here
synchronises.  There is no CPU path.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib


class _IouAttrs(ctypes.Structure):
    _fields_ = [("eps", ctypes.c_float)]


class _NmsAttrs(ctypes.Structure):
    _fields_ = [("iou_threshold", ctypes.c_float), ("eps", ctypes.c_float), ("mode", ctypes.c_int32),
                ("max_output", ctypes.c_int32)]


NMS_MODE_JIT = 0      # nms_jit: suppress iff ovr >= thr, eps on w/h/area
NMS_MODE_PLUS1 = 1    # apply_nms: +1 pixel convention, suppress iff ovr > thr
NMS_MODE_STRICT = 2   # suppress iff IoU > thr, union clamped at 1e-8


def _f32c(t):
    return t.contiguous().to(torch.float32)


def _thresh_tensor(thresh, device):
    if isinstance(thresh, torch.Tensor):
        return thresh.to(device=device, dtype=torch.float32).reshape(1).contiguous()
    return torch.full((1,), float(thresh), dtype=torch.float32, device=device)


# ----------------------------------------------------------------------------- AOT-op "cells"
class NMS:
    """Mirror of det3d_ms.ops.nms_cpu.NMS, executed on the GPU (boxes_iou_nms_gpu)."""

    def __call__(self, boxes, thresh):
        boxes = _f32c(boxes)
        n = boxes.shape[0]
        keep = torch.empty((n,), dtype=torch.int32, device=boxes.device)
        num = torch.empty((1,), dtype=torch.int32, device=boxes.device)
        _lib.call("boxes_iou_nms_gpu", [boxes, _thresh_tensor(thresh, boxes.device), keep, num])
        return keep, num[0]

    construct = __call__


class _PairMatrix:
    _sym = None

    def __call__(self, a, b):
        a, b = _f32c(a), _f32c(b)
        out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
        _lib.call(self._sym, [a, b, out])
        return out

    construct = __call__


class BoxesIouBevGpu(_PairMatrix):
    _sym = "BoxesIouBevGpu"


class BoxesOverlapBevGpu(_PairMatrix):
    _sym = "BoxesOverlapBevGpu"


class _NmsCell:
    _sym = None

    def __call__(self, boxes, thresh):
        boxes = _f32c(boxes)
        n = boxes.shape[0]
        keep = torch.empty((n,), dtype=torch.int64, device=boxes.device)
        num = torch.empty((1,), dtype=torch.int32, device=boxes.device)
        _lib.call(self._sym, [boxes, _thresh_tensor(thresh, boxes.device), keep, num])
        return keep, num

    construct = __call__


class NumGpu(_NmsCell):  # (sic) the reference's class name for NmsGpu, iou_gpu.py:51
    _sym = "NmsGpu"


NmsGpu = NumGpu


class NmsNormalGpu(_NmsCell):
    _sym = "NmsNormalGpu"


# ----------------------------------------------------------------------------- iou3d_nms_utils mirror
def boxes_iou_bev(boxes_a, boxes_b):
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return BoxesIouBevGpu()(boxes_a, boxes_b)


def boxes_overlap_bev(boxes_a, boxes_b):
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return BoxesOverlapBevGpu()(boxes_a, boxes_b)


def to_pcdet(boxes):
    boxes = boxes[:, [0, 1, 2, 4, 3, 5, -1]].clone()
    boxes[:, -1] = -boxes[:, -1] - math.pi / 2
    return boxes


def boxes_iou3d_gpu(boxes_a, boxes_b):
    """iou3d_nms_utils.py:40-81: BEV overlap x height overlap / volume union."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    boxes_a, boxes_b = to_pcdet(boxes_a), to_pcdet(boxes_b)
    a_max = (boxes_a[:, 2] + boxes_a[:, 5] / 2).view(-1, 1)
    a_min = (boxes_a[:, 2] - boxes_a[:, 5] / 2).view(-1, 1)
    b_max = (boxes_b[:, 2] + boxes_b[:, 5] / 2).view(1, -1)
    b_min = (boxes_b[:, 2] - boxes_b[:, 5] / 2).view(1, -1)
    overlaps_bev = boxes_overlap_bev(boxes_a.contiguous(), boxes_b.contiguous())
    overlaps_h = torch.clamp(torch.min(a_max, b_max) - torch.max(a_min, b_min), min=0)
    overlaps_3d = overlaps_bev * overlaps_h
    vol_a = (boxes_a[:, 3] * boxes_a[:, 4] * boxes_a[:, 5]).view(-1, 1)
    vol_b = (boxes_b[:, 3] * boxes_b[:, 4] * boxes_b[:, 5]).view(1, -1)
    return overlaps_3d / torch.clamp(vol_a + vol_b - overlaps_3d, min=1e-6)


def _sorted_order(scores):
    # stable descending sort: ties keep the lower index first (SURVEY 8c TopK definition)
    return torch.sort(scores, dim=0, descending=True, stable=True)[1]


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """iou3d_nms_utils.py:84-99: returns (indices into the ORIGINAL boxes, None)."""
    assert boxes.shape[1] == 7
    order = _sorted_order(scores)
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    keep, num = NumGpu()(boxes[order].contiguous(), thresh)
    return order[keep[: int(num.item())]].contiguous(), None


def nms_normal_gpu(boxes, scores, thresh, **kwargs):
    """iou3d_nms_utils.py:102-116."""
    assert boxes.shape[1] == 7
    order = _sorted_order(scores)
    keep, num = NmsNormalGpu()(boxes[order].contiguous(), thresh)
    return order[keep[: int(num.item())]].contiguous(), None


# ----------------------------------------------------------------------------- axis-aligned
def iou_jit(boxes, query_boxes, eps=0.0):
    boxes, query_boxes = _f32c(boxes), _f32c(query_boxes)
    out = torch.empty((boxes.shape[0], query_boxes.shape[0]), dtype=torch.float32, device=boxes.device)
    _lib.call("md_iou_aligned", [boxes, query_boxes, out], extra=_IouAttrs(float(eps)))
    return out


def nms_aligned(boxes_sorted, thresh, eps=0.0, mode=NMS_MODE_JIT, count=None, group=None, max_output=0,
                workspace=None):
    """Greedy NMS over score-sorted corner boxes [N,4] or a batch [B,N,4].

    Returns (keep_mask u8, keep_idx i32 zero-padded, num i32[B])."""
    b = _f32c(boxes_sorted)
    batched = b.dim() == 3
    B, n = (b.shape[0], b.shape[1]) if batched else (1, b.shape[0])
    dev = b.device
    mask = torch.empty((B, n) if batched else (n,), dtype=torch.uint8, device=dev)
    idx = torch.empty((B, n) if batched else (n,), dtype=torch.int32, device=dev)
    num = torch.empty((B,), dtype=torch.int32, device=dev)
    if count is not None:
        count = count.to(device=dev, dtype=torch.int32).reshape(B).contiguous()
    if group is not None:
        group = group.to(device=dev, dtype=torch.int32).contiguous()
    params = [b, count, group, mask, idx, num]
    if workspace is None and B * n > 0:
        # suppression-mask scratch from torch's caching allocator (never blocks), not from the op's hipMallocAsync fallback
        workspace = _lib.scratch("md_nms_aligned", (B, n, max(int(max_output), 0)), dev)
    if workspace is not None:
        params.append(workspace)
    _lib.call("md_nms_aligned", params, extra=_NmsAttrs(float(thresh), float(eps), int(mode), int(max_output)))
    return mask, idx, num


def nms_jit(dets, thresh, eps=0.0):
    """pointpillars/src/core/nms.py:85-112 on device: dets [N,5] (x1,y1,x2,y2,score) -> keep
    indices (original numbering, score order), as a device int64 tensor."""
    order = _sorted_order(dets[:, 4])
    _, idx, num = nms_aligned(dets[order, :4].contiguous(), thresh, eps, NMS_MODE_JIT)
    return order[idx[: int(num.item())].long()]


def circle_nms(dets, thresh):
    """dets [N,3] = x, y, score. Returns keep indices in the original numbering."""
    order = _sorted_order(dets[:, 2])
    xy = _f32c(dets[order, :2])
    n = xy.shape[0]
    mask = torch.empty((n,), dtype=torch.uint8, device=xy.device)
    idx = torch.empty((n,), dtype=torch.int32, device=xy.device)
    num = torch.empty((1,), dtype=torch.int32, device=xy.device)
    _lib.call("md_circle_nms", [xy, _thresh_tensor(thresh, xy.device), mask, idx, num])
    return order[idx[: int(num.item())].long()]


# ----------------------------------------------------------------------------- anchors / codecs / select / roialign
class _FpnAnchorAttrs(ctypes.Structure):
    _fields_ = [("num_levels", ctypes.c_int32), ("num_ratios", ctypes.c_int32), ("feat_h", ctypes.c_int32 * 8),
                ("feat_w", ctypes.c_int32 * 8), ("stride", ctypes.c_int32 * 8), ("scale", ctypes.c_float),
                ("ratios", ctypes.c_float * 16)]


class _Anchor3dAttrs(ctypes.Structure):
    _fields_ = [("feat_h", ctypes.c_int32), ("feat_w", ctypes.c_int32), ("num_rot", ctypes.c_int32),
                ("range", ctypes.c_double * 6), ("z_offset", ctypes.c_double), ("size", ctypes.c_double * 3),
                ("rotations", ctypes.c_double * 8), ("slot_off", ctypes.c_int32), ("slots_total", ctypes.c_int32)]


class _Anchor3dRangeAttrs(ctypes.Structure):
    _fields_ = [("feat_d", ctypes.c_int32), ("feat_h", ctypes.c_int32), ("feat_w", ctypes.c_int32), ("num_sizes", ctypes.c_int32),
                ("num_rot", ctypes.c_int32), ("linspace_mode", ctypes.c_int32), ("slot_off", ctypes.c_int32),
                ("slots_total", ctypes.c_int32), ("range", ctypes.c_double * 6), ("sizes", (ctypes.c_double * 3) * 4),
                ("rotations", ctypes.c_double * 8)]


class _AnchorMaskAttrs(ctypes.Structure):
    _fields_ = [("grid_x", ctypes.c_int32), ("grid_y", ctypes.c_int32), ("voxel_x", ctypes.c_float),
                ("voxel_y", ctypes.c_float), ("offset_x", ctypes.c_float), ("offset_y", ctypes.c_float),
                ("area_threshold", ctypes.c_float)]


class _DeltaAttrs(ctypes.Structure):
    _fields_ = [("means", ctypes.c_float * 4), ("stds", ctypes.c_float * 4), ("max_ratio", ctypes.c_float),
                ("clip_w", ctypes.c_float), ("clip_h", ctypes.c_float)]


class _TopkAttrs(ctypes.Structure):
    _fields_ = [("k", ctypes.c_int32), ("min_score", ctypes.c_float), ("max_segment", ctypes.c_int32)]


class _RoiAlignAttrs(ctypes.Structure):
    _fields_ = [("num_levels", ctypes.c_int32), ("pooled", ctypes.c_int32), ("sampling_ratio", ctypes.c_int32),
                ("aligned", ctypes.c_int32), ("k_min", ctypes.c_int32), ("canonical_level", ctypes.c_int32),
                ("canonical_scale", ctypes.c_float), ("spatial_scale", ctypes.c_float * 6)]


class _ClipAttrs(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_float), ("hi", ctypes.c_float)]


FLT_MAX = 3.4028234663852886e38


def fpn_anchors(feat_sizes, strides=(4, 8, 16, 32, 64), scale=8.0, ratios=(0.5, 1.0, 2.0), device="cuda"):
    at = _FpnAnchorAttrs()
    at.num_levels, at.num_ratios, at.scale = len(feat_sizes), len(ratios), float(scale)
    total = 0
    for i, ((h, w), s) in enumerate(zip(feat_sizes, strides)):
        at.feat_h[i], at.feat_w[i], at.stride[i] = int(h), int(w), int(s)
        total += h * w * len(ratios)
    for i, r in enumerate(ratios):
        at.ratios[i] = float(r)
    out = torch.empty((total, 4), dtype=torch.float32, device=device)
    _lib.call("md_anchors_fpn", [out], extra=at)
    return out


def create_anchors_3d_stride(feature_size, sizes=(1.6, 3.9, 1.56), anchor_strides=(0.4, 0.4, 0.0),
                             anchor_offsets=(0.2, -39.8, -1.78), rotations=(0, math.pi / 2),
                             anchor_range=(0.0, -39.68, -3.0, 69.12, 39.68, 1.0), dtype=torch.float32, device="cuda", out=None, slot_off=0):
    """pointpillars/src/core/box_np_ops.py:453-523 on device: returns [1,H,W,1,R,7] fp32.
    (anchor_strides / x,y offsets are unused by the reference too: it derives the stride from
    anchor_range, :476-477.)  out [1,H,W,slots,7] + slot_off: write rows [slot_off, slot_off + R) of a concatenated table."""
    d, h, w = feature_size
    assert d == 1 and len(rotations) == 2, "the reference hard-codes one z slice and two rotations (:492)"
    at = _Anchor3dAttrs()
    at.feat_h, at.feat_w, at.num_rot = int(h), int(w), len(rotations)
    for i in range(6):
        at.range[i] = float(anchor_range[i])
    at.z_offset = float(anchor_offsets[2])
    flat = [float(v) for v in (sizes if not isinstance(sizes[0], (list, tuple)) else sizes[0])]
    for i in range(3):
        at.size[i] = flat[i]
    for i, r in enumerate(rotations):
        at.rotations[i] = float(r)
    if out is None:
        out = torch.empty((1, h, w, 1, len(rotations), 7), dtype=torch.float32, device=device)
    else:
        at.slot_off, at.slots_total = int(slot_off), int(out.shape[-2])
    _lib.call("md_anchors_3d_stride", [out], extra=at)
    return out


def create_anchors_3d_range(feature_size, anchor_range, sizes=(1.6, 3.9, 1.56), rotations=(0, math.pi / 2), device="cuda",
                            linspace_mode=0, out=None, slot_off=0):
    """pointpillars/src/core/box_np_ops.py:526-568 on device: [D,H,W,S,R,7] fp32, centres on np.linspace(lo, hi, n) per axis.
    linspace_mode: md_anchor3d_range_attrs (0 = the float32 arithmetic of numpy >= 2, 1 = numpy 1.21's float64)."""
    d, h, w = [int(v) for v in feature_size]
    flat = [float(v) for row in (sizes if isinstance(sizes[0], (list, tuple)) else [sizes]) for v in row]
    ns = len(flat) // 3
    at = _Anchor3dRangeAttrs()
    at.feat_d, at.feat_h, at.feat_w, at.num_sizes, at.num_rot, at.linspace_mode = d, h, w, ns, len(rotations), int(linspace_mode)
    for i in range(6):
        at.range[i] = float(anchor_range[i])
    for k in range(ns):
        for i in range(3):
            at.sizes[k][i] = flat[3 * k + i]
    for i, r in enumerate(rotations):
        at.rotations[i] = float(r)
    if out is None:
        out = torch.empty((d, h, w, ns, len(rotations), 7), dtype=torch.float32, device=device)
    else:
        at.slot_off, at.slots_total = int(slot_off), int(out.shape[-2])
    _lib.call("md_anchors_3d_range", [out], extra=at)
    return out


class AnchorGeneratorStride:
    """pointpillars/src/core/anchor_generator.py:6-63 (same constructor arguments and properties); generate() runs on the device."""

    def __init__(self, sizes=(1.6, 3.9, 1.56), anchor_strides=(0.4, 0.4, 1.0), anchor_offsets=(0.2, -39.8, -1.78),
                 rotations=(0, math.pi / 2), class_id=None, match_threshold=-1, unmatch_threshold=-1,
                 anchor_range=(0.0, -39.68, -3.0, 69.12, 39.68, 1.0)):
        self._sizes, self._anchor_strides, self._anchor_offsets, self._rotations = sizes, anchor_strides, anchor_offsets, rotations
        self.class_id, self.match_threshold, self.unmatch_threshold = class_id, match_threshold, unmatch_threshold
        self.anchor_range = anchor_range

    @property
    def num_anchors_per_localization(self):
        flat = self._sizes if isinstance(self._sizes[0], (list, tuple)) else [self._sizes]
        return len(self._rotations) * len(flat)

    def generate(self, feature_map_size, device="cuda", out=None, slot_off=0):
        return create_anchors_3d_stride(feature_map_size, self._sizes, self._anchor_strides, self._anchor_offsets, self._rotations,
                                        self.anchor_range, device=device, out=out, slot_off=slot_off)


def generate_anchors(anchor_generators, feature_map_size, device="cuda"):
    """TargetAssigner.generate_anchors (pointpillars/src/core/target_assigner.py:227-249): every generator's anchors reshaped to
    [*shape[:3], -1, 7] and concatenated on axis -2, with the per-anchor matched / unmatched thresholds of its generator.  Each
    generator writes its rows of the concatenated table in place (no concat copy).  The threshold vectors are ordered as the
    reference builds them: generator after generator (np.concatenate of np.full blocks), NOT in the anchor table's order."""
    d, h, w = [int(v) for v in feature_map_size]
    per = [g.num_anchors_per_localization for g in anchor_generators]
    out = torch.empty((d, h, w, sum(per), 7), dtype=torch.float32, device=device)
    off = 0
    for g, n in zip(anchor_generators, per):
        g.generate(feature_map_size, device=device, out=out, slot_off=off)
        off += n
    locs = d * h * w
    matched = torch.cat([torch.full((locs * n,), float(g.match_threshold), dtype=torch.float32) for g, n in zip(anchor_generators, per)])
    unmatched = torch.cat([torch.full((locs * n,), float(g.unmatch_threshold), dtype=torch.float32) for g, n in zip(anchor_generators, per)])
    return {"anchors": out, "matched_thresholds": matched.to(device), "unmatched_thresholds": unmatched.to(device)}


def anchors_mask(coors, grid_size_xy, anchors_bv, voxel_size, pc_range, area_threshold):
    """preprocess.py:211-225: (anchors_area f32, anchors_mask bool) for one sample."""
    at = _AnchorMaskAttrs(int(grid_size_xy[0]), int(grid_size_xy[1]), float(voxel_size[0]), float(voxel_size[1]),
                          float(pc_range[0]), float(pc_range[1]), float(area_threshold))
    coors = coors.to(torch.int32).contiguous()
    bv = _f32c(anchors_bv)
    area = torch.empty((bv.shape[0],), dtype=torch.float32, device=bv.device)
    mask = torch.empty((bv.shape[0],), dtype=torch.uint8, device=bv.device)
    _lib.call("md_anchor_mask", [coors, bv, area, mask], extra=at)
    return area, mask.bool()


def rbbox2d_to_near_bbox(rbboxes):
    """pointpillars/src/core/box_np_ops.py:180-192: rotated BEV boxes [N,5] (x, y, dx, dy, r) -> the nearest axis-aligned boxes
    [N,4] (xmin, ymin, xmax, ymax): dx and dy change places where the rotation, folded into [-pi/2, pi/2), is beyond pi/4."""
    r = _f32c(rbboxes)
    rot = r[:, 4]
    folded = (rot - torch.floor(rot / math.pi + 0.5) * math.pi).abs()
    dims = torch.where((folded > math.pi / 4).unsqueeze(1), r[:, [3, 2]], r[:, 2:4])
    return torch.cat([r[:, :2] - dims / 2, r[:, :2] + dims / 2], 1).contiguous()


def second_box_decode(box_encodings, anchors):
    enc, anc = _f32c(box_encodings), _f32c(anchors).reshape(-1, 7)
    out = torch.empty_like(enc)
    _lib.call("md_second_box_decode", [enc, anc, out])
    return out


def delta2bbox(rois, deltas, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), max_shape=None, wh_ratio_clip=16 / 1000):
    at = _decode_attrs(means, stds, max_shape, wh_ratio_clip)
    rois, deltas = _f32c(rois), _f32c(deltas)
    out = torch.empty_like(rois)
    _lib.call("md_delta2bbox", [rois, deltas, out], extra=at)
    return out


def topk_segmented(scores, seg_offsets, k, min_score=None, out_cnt=None, max_segment=None):
    """scores [T] f32, seg_offsets [L+1] i32 (device) -> (values [L,k], indices [L,k] i32, count [L])."""
    scores = _f32c(scores).reshape(-1)
    L = seg_offsets.numel() - 1
    vals = torch.empty((L, k), dtype=torch.float32, device=scores.device)
    idx = torch.empty((L, k), dtype=torch.int32, device=scores.device)
    cnt = out_cnt if out_cnt is not None else torch.empty((L,), dtype=torch.int32, device=scores.device)
    max_segment = int(scores.numel() if max_segment is None else max_segment)
    params = [scores, seg_offsets, vals, idx, cnt]
    dims = (L, int(k), max_segment)
    if min(dims) >= 0 and _lib.workspace_bytes("md_topk_segmented", *dims):
        # the multi-workgroup select takes scratch: hand it a block of torch's caching allocator.  Without it the op falls back to
        # hipMallocAsync / hipFreeAsync, which BLOCKED the host ~7 ms per call on ROCm 7.2 (r03 tools/host_enqueue.py: 49.6 of the
        # 51.9 ms the host spent enqueuing one Faster R-CNN step sat in these seven calls, the device queue running dry behind each)
        params.append(_lib.scratch("md_topk_segmented", dims, scores.device))
    _lib.call("md_topk_segmented", params,
              extra=_TopkAttrs(int(k), -FLT_MAX if min_score is None else float(min_score), max_segment))
    return vals, idx, cnt


def top_k(scores2d, k):
    """ops.TopK(sorted=True) on the last axis of a [L, n] tensor."""
    L, n = scores2d.shape
    off = torch.arange(0, (L + 1) * n, n, dtype=torch.int32, device=scores2d.device)
    v, i, _ = topk_segmented(scores2d.contiguous(), off, k, max_segment=n)
    return v, i


def roi_align(feats, rois, out_size=7, spatial_scales=None, sampling_ratio=2, aligned=True, k_min=2,
              canonical_level=4, canonical_scale=224.0, return_levels=False):
    """feats: list of [N,H,W,C] bf16 NHWC levels; rois [R,5] (batch_idx,x1,y1,x2,y2) -> [R,P,P,C] bf16."""
    L = len(feats)
    at = _RoiAlignAttrs()
    at.num_levels, at.pooled, at.sampling_ratio, at.aligned = L, int(out_size), int(sampling_ratio), int(aligned)
    at.k_min, at.canonical_level, at.canonical_scale = int(k_min), int(canonical_level), float(canonical_scale)
    for i in range(L):
        at.spatial_scale[i] = float(spatial_scales[i])
    rois = _f32c(rois)
    R, C = rois.shape[0], feats[0].shape[3]
    out = torch.empty((R, out_size, out_size, C), dtype=torch.bfloat16, device=rois.device)
    lv = torch.empty((R,), dtype=torch.int32, device=rois.device) if return_levels else None
    _lib.call("md_roi_align", [rois] + list(feats) + [out, lv], extra=at)
    return (out, lv) if return_levels else out


def sigmoid_clip(x, lo=1e-4, hi=1 - 1e-4):
    x = _f32c(x)
    y = torch.empty_like(x)
    _lib.call("md_sigmoid_clip", [x, y], extra=_ClipAttrs(lo, hi))
    return y


class _PeakAttrs(ctypes.Structure):
    _fields_ = [("c0", ctypes.c_int32), ("num_classes", ctypes.c_int32), ("lo", ctypes.c_float), ("hi", ctypes.c_float)]


def heat_peaks(head, c0, num_classes, with_hm=False, lo=1e-4, hi=1 - 1e-4):
    """head [B,H,W,Cp] bf16 NHWC -> (heat [B,nc,H,W] f32 = sigmoid-clipped heat map zeroed off its 3x3 maxima, hm or None):
    nhwc_to_nchw_f32 + sigmoid_clip + md_heat_nms in one md_heat_peaks launch, bit-identical to the three."""
    b, h, w, _ = head.shape
    heat = torch.empty((b, num_classes, h, w), dtype=torch.float32, device=head.device)
    hm = torch.empty_like(heat) if with_hm else None
    _lib.call("md_heat_peaks", [head, heat, hm], extra=_PeakAttrs(int(c0), int(num_classes), float(lo), float(hi)))
    return heat, hm


class DetectionDecode:
    """Mirror of centernet/src/decode.py:123-196 (NMS :40-64, GatherTopK :90-109): feature dict with
    'hm' [B,C,H,W] (already sigmoid+clip), 'wh', 'reg' [B,2,H,W] fp32 NCHW -> detections [B,K,6]."""

    def __init__(self, reg_offset=True, K=100):
        self.reg_offset, self.K = reg_offset, K

    def __call__(self, feature, return_indices=False):
        wh = _f32c(feature["wh"])
        reg = _f32c(feature["reg"]) if self.reg_offset else None
        K = self.K
        if feature.get("heat") is not None:      # peaks already extracted (heat_peaks: the fused head post-processing)
            heat = _f32c(feature["heat"])
        else:
            hm = _f32c(feature["hm"])
            heat = torch.empty_like(hm)
            _lib.call("md_heat_nms", [hm, heat])
        B, C, H, W = heat.shape
        v1, i1 = top_k(heat.view(B * C, H * W), K)           # per-class top-K  (decode.py:96)
        v2, i2 = top_k(v1.view(B, C * K), K)                 # global top-K     (decode.py:101)
        det = torch.empty((B, K, 6), dtype=torch.float32, device=heat.device)
        inds = torch.empty((B, K), dtype=torch.int32, device=heat.device)
        cls = torch.empty((B, K), dtype=torch.int32, device=heat.device)
        _lib.call("md_centernet_assemble", [v2, i2, i1.view(B, C, K), wh, reg, det, inds, cls])
        return (det, inds, cls) if return_indices else det

    construct = __call__


# ----------------------------------------------------------------------------- two-stage glue
class _RpnDecodeAttrs(ctypes.Structure):
    _fields_ = [("num_anchors", ctypes.c_int32), ("decode", _DeltaAttrs)]


class _RcnnAttrs(ctypes.Structure):
    _fields_ = [("num_classes", ctypes.c_int32), ("reg_offset", ctypes.c_int32), ("score_thr", ctypes.c_float),
                ("decode", _DeltaAttrs)]


def _decode_attrs(means, stds, img_hw, wh_ratio_clip=16 / 1000):
    at = _DeltaAttrs()
    for i in range(4):
        at.means[i], at.stds[i] = float(means[i]), float(stds[i])
    at.max_ratio = abs(math.log(wh_ratio_clip))
    at.clip_h, at.clip_w = (float(img_hw[0]), float(img_hw[1])) if img_hw is not None else (0.0, 0.0)
    return at


def rpn_decode(head, anchors, idx, cnt, num_anchors, img_hw, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), out_boxes=None,
               out_scores=None):
    B, k = idx.shape
    if out_boxes is None:
        out_boxes = torch.empty((B, k, 4), dtype=torch.float32, device=head.device)
    if out_scores is None:
        out_scores = torch.empty((B, k), dtype=torch.float32, device=head.device)
    at = _RpnDecodeAttrs(int(num_anchors), _decode_attrs(means, stds, img_hw))
    _lib.call("md_rpn_decode", [head, anchors, idx, cnt, out_boxes, out_scores], extra=at)
    return out_boxes, out_scores


def rpn_merge(boxes, scores, keep):
    L, B, k = scores.shape
    mboxes = torch.empty((B, L * k, 4), dtype=torch.float32, device=boxes.device)
    mscores = torch.empty((B, L * k), dtype=torch.float32, device=boxes.device)
    _lib.call("md_rpn_merge", [boxes, scores, keep, mboxes, mscores])
    return mboxes, mscores


def make_rois(mboxes, topv, topi, cnt):
    B, post = topv.shape
    rois = torch.empty((B * post, 5), dtype=torch.float32, device=mboxes.device)
    rs = torch.empty((B * post,), dtype=torch.float32, device=mboxes.device)
    _lib.call("md_make_rois", [mboxes, topv, topi, cnt, rois, rs])
    return rois, rs


def rcnn_scores(cls_reg, roi_cnt, num_classes, score_thr):
    R = cls_reg.shape[0]
    B = roi_cnt.numel()
    cand = torch.empty((B, (R // B) * num_classes), dtype=torch.float32, device=cls_reg.device)
    at = _RcnnAttrs(int(num_classes), 0, float(score_thr), _DeltaAttrs())
    _lib.call("md_rcnn_scores", [cls_reg, roi_cnt, cand], extra=at)
    return cand


def rcnn_decode_selected(cls_reg, rois, sel_idx, sel_cnt, num_classes, reg_offset, img_hw, means=(0, 0, 0, 0),
                         stds=(0.1, 0.1, 0.2, 0.2)):
    B, npre = sel_idx.shape
    boxes = torch.empty((B, npre, 4), dtype=torch.float32, device=cls_reg.device)
    labels = torch.empty((B, npre), dtype=torch.int32, device=cls_reg.device)
    at = _RcnnAttrs(int(num_classes), int(reg_offset), 0.0, _decode_attrs(means, stds, img_hw))
    _lib.call("md_rcnn_decode_selected", [cls_reg, rois, sel_idx, sel_cnt, boxes, labels], extra=at)
    return boxes, labels


def pack_detections(boxes, scores, labels, keep_idx, num, max_det, sel_cnt=None, status=None):
    """-> dets [B,max_det,6], count [B].  With sel_cnt (the pre-NMS top-k's counts) and status ([B] int32, caller-cleared, in/out)
    bit 0 of status[b] is OR-ed in when the top-npre prefix was full AND gave fewer than max_det survivors: only then can the cut
    differ from the NMS over every candidate (see PrefixStatus)."""
    B = scores.shape[0]
    dets = torch.empty((B, max_det, 6), dtype=torch.float32, device=boxes.device)
    count = torch.empty((B,), dtype=torch.int32, device=boxes.device)
    if status is None:
        _lib.call("md_pack_detections", [boxes, scores, labels, keep_idx, num, dets, count])
    else:
        _lib.call("md_pack_detections", [boxes, scores, labels, keep_idx, num, sel_cnt, dets, count, status])
    return dets, count


class PrefixStatus:
    """Per-image sticky flags of the pre-NMS prefix cut (md_pack_detections, 9-parameter form), kept on the device: the hot path
    never synchronises for them; `flagged()` reads them (one host sync) when the caller wants to know, `clear()` resets."""

    def __init__(self):
        self._t = {}

    def tensor(self, batch, device):
        # one flag tensor per (batch, device, HIP stream): two streams running parts of a batch (graphs.SplitForward) never share a row
        key = (int(batch), str(device), torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0)
        if key not in self._t:
            self._t[key] = torch.zeros((batch,), dtype=torch.int32, device=device)
        return self._t[key]

    def flagged(self):
        """image slots (of any batch size seen) whose result MAY differ from the untruncated class-wise NMS."""
        return int(sum(int((t & 1).sum().item()) for t in self._t.values()))

    def clear(self):
        for t in self._t.values():
            t.zero_()


# ----------------------------------------------------------------------------- CenterPoint head post-processing
class _CenterPointAttrs(ctypes.Structure):
    _fields_ = [("off_reg", ctypes.c_int32), ("off_height", ctypes.c_int32), ("off_dim", ctypes.c_int32),
                ("off_rot", ctypes.c_int32), ("off_vel", ctypes.c_int32), ("off_hm", ctypes.c_int32),
                ("num_classes", ctypes.c_int32), ("score_threshold", ctypes.c_float), ("out_size_factor", ctypes.c_float),
                ("voxel_size", ctypes.c_float * 2), ("pc_range", ctypes.c_float * 2), ("post_center_range", ctypes.c_float * 6)]


def gather_rows(src, idx, cnt=None):
    """src [B,n,W] f32, idx [B,k] i32 -> [B,k,W] (zero rows past cnt)."""
    B, k = idx.shape
    out = torch.empty((B, k, src.shape[2]), dtype=torch.float32, device=src.device)
    _lib.call("md_gather_rows", [src, idx, cnt, out])
    return out


class CenterHeadPost:
    """Mirror of CenterHead.predict + post_processing for ONE task
    (centerpoint/det3d_ms/models/bbox_heads/center_head.py:273-463): decode every BEV cell, mask by score and
    post_center_range, TopK(nms_pre_max_size), rotated NMS through the AOT operator's device twin
    (`self.nms(boxes_for_nms_sorted, thr)`, :443-445), count = min(num_out, mask_num, nms_post_max_size)."""

    def __init__(self, offsets, num_classes, test_cfg):
        self.off, self.nc, self.cfg = dict(offsets), int(num_classes), test_cfg

    def __call__(self, head, return_aux=False):
        B, H, W, C = head.shape
        cfg = self.cfg
        at = _CenterPointAttrs()
        at.off_reg, at.off_height, at.off_dim, at.off_rot = self.off["reg"], self.off["height"], self.off["dim"], self.off["rot"]
        at.off_vel, at.off_hm, at.num_classes = self.off.get("vel", -1), self.off["hm"], self.nc
        at.score_threshold, at.out_size_factor = float(cfg["score_threshold"]), float(cfg["out_size_factor"])
        for i in range(2):
            at.voxel_size[i], at.pc_range[i] = float(cfg["voxel_size"][i]), float(cfg["pc_range"][i])
        for i in range(6):
            at.post_center_range[i] = float(cfg["post_center_limit_range"][i])
        dev = head.device
        n = H * W
        scores = torch.empty((B, n), dtype=torch.float32, device=dev)
        labels = torch.empty((B, n), dtype=torch.int32, device=dev)
        boxes = torch.empty((B, n, 9), dtype=torch.float32, device=dev)
        nms_boxes = torch.empty((B, n, 7), dtype=torch.float32, device=dev)
        _lib.call("md_centerpoint_decode", [head, scores, labels, boxes, nms_boxes], extra=at)
        k = int(cfg["nms"]["nms_pre_max_size"])
        sc_sorted, order = top_k(scores, k)                       # TopK over ALL cells, masked ones carry -1 (:435)
        nb_sorted = gather_rows(nms_boxes, order)
        bx_sorted = gather_rows(boxes, order)
        mask_num = (sc_sorted > -1.0).sum(1).to(torch.int32)      # == mask[order].sum() (:439-441)
        nms = NMS()
        keeps, nums = [], []
        for b in range(B):                                       # the reference loops the batch too (:405)
            kp, nm = nms(nb_sorted[b], cfg["nms"]["nms_iou_threshold"])
            keeps.append(kp)
            nums.append(nm.reshape(1))
        keep = torch.stack(keeps)
        num_out = torch.cat(nums)
        count = torch.minimum(torch.minimum(num_out, mask_num), torch.full_like(num_out, int(cfg["nms"]["nms_post_max_size"])))
        sel_boxes = gather_rows(bx_sorted, keep)
        sel_scores = torch.gather(sc_sorted, 1, keep.long())
        sel_labels = torch.gather(torch.gather(labels, 1, order.long()), 1, keep.long())
        out = [sel_boxes, sel_scores, sel_labels, count]
        if return_aux:
            return out, dict(scores=scores, labels=labels, boxes=boxes, nms_boxes=nms_boxes, order=order, keep=keep,
                             num_out=num_out, mask_num=mask_num)
        return out


class _NmsRotatedAttrs(ctypes.Structure):
    _fields_ = [("iou_threshold", ctypes.c_float), ("mode", ctypes.c_int32), ("max_output", ctypes.c_int32)]


NMS_ROT_GPU = 0       # NmsGpu: suppress iff so / max(sa + sb - so, 1e-8) > thr
NMS_ROT_CPU = 1       # boxes_iou_nms_cpu: suppress iff so / (sa + sb - so) >= thr; zero-area boxes are dropped up front


def nms_rotated(boxes, thresh, mode, count=None, max_output=0, workspace=None):
    """Greedy rotated-BEV NMS over score-sorted boxes [N,7] or L lists [L,N,7] in one call (md_nms_rotated, include/minddet_hip_cp.h);
    count [L] int32: the valid leading rows per list (None: all).  Returns (keep_idx i32 zero-padded, num i32 [L])."""
    b = _f32c(boxes)
    batched = b.dim() == 3
    L, n = (b.shape[0], b.shape[1]) if batched else (1, b.shape[0])
    dev = b.device
    idx = torch.empty((L, n) if batched else (n,), dtype=torch.int32, device=dev)
    num = torch.empty((L,), dtype=torch.int32, device=dev)
    if count is not None:
        count = count.to(device=dev, dtype=torch.int32).reshape(L).contiguous()
    params = [b, count, idx, num]
    if workspace is None and L * n > 0:
        # record + mask scratch from torch's caching allocator (never blocks), as nms_aligned does
        workspace = _lib.scratch("md_nms_rotated", (L, n), dev)
    if workspace is not None:
        params.append(workspace)
    _lib.call("md_nms_rotated", params, extra=_NmsRotatedAttrs(float(thresh), int(mode), int(max_output)))
    return idx, num


CP_MAX_TASKS = 8


class _CPTaskAttrs(ctypes.Structure):
    _fields_ = [("off_reg", ctypes.c_int32), ("off_height", ctypes.c_int32), ("off_dim", ctypes.c_int32), ("off_rot", ctypes.c_int32),
                ("off_vel", ctypes.c_int32), ("off_hm", ctypes.c_int32), ("num_classes", ctypes.c_int32), ("class_base", ctypes.c_int32)]


class _CPHeadAttrs(ctypes.Structure):
    _fields_ = [("num_tasks", ctypes.c_int32), ("task", _CPTaskAttrs * CP_MAX_TASKS), ("score_threshold", ctypes.c_float),
                ("out_size_factor", ctypes.c_float), ("voxel_size", ctypes.c_float * 2), ("pc_range", ctypes.c_float * 2),
                ("post_center_range", ctypes.c_float * 6), ("max_per_task", ctypes.c_int32)]


def cp_head_attrs(task_offsets, num_classes, test_cfg):
    """md_cp_head_attrs of a CenterHead (per task {head: first channel}, per task num_class) under a test config"""
    if not 1 <= len(task_offsets) <= CP_MAX_TASKS or len(task_offsets) != len(num_classes):
        raise ValueError(f"cp_head_attrs: 1 .. {CP_MAX_TASKS} tasks, one num_class each; got {len(task_offsets)} / {len(num_classes)}")
    at = _CPHeadAttrs()
    at.num_tasks = len(task_offsets)
    base = 0
    for t, (off, nc) in enumerate(zip(task_offsets, num_classes)):
        a = at.task[t]
        a.off_reg, a.off_height, a.off_dim, a.off_rot = int(off["reg"]), int(off["height"]), int(off["dim"]), int(off["rot"])
        a.off_vel, a.off_hm, a.num_classes, a.class_base = int(off.get("vel", -1)), int(off["hm"]), int(nc), base
        base += int(nc)
    at.score_threshold, at.out_size_factor = float(test_cfg["score_threshold"]), float(test_cfg["out_size_factor"])
    for i in range(2):
        at.voxel_size[i], at.pc_range[i] = float(test_cfg["voxel_size"][i]), float(test_cfg["pc_range"][i])
    for i in range(6):
        at.post_center_range[i] = float(test_cfg["post_center_limit_range"][i])
    at.max_per_task = int(test_cfg["nms"]["nms_post_max_size"])
    return at


def cp_scores(head, at):
    """head [B,H,W,C] bf16 -> scores [B,T,H W] f32: per cell and task the first maximum of the class sigmoids, -1 where the score or
    the range mask fails (md_cp_scores)"""
    B, H, W, _ = head.shape
    scores = torch.empty((B, at.num_tasks, H * W), dtype=torch.float32, device=head.device)
    _lib.call("md_cp_scores", [head, scores], extra=at)
    return scores


def cp_decode_selected(head, idx, cnt, at):
    """idx [B,T,k] i32 (cell per selected row), cnt [B,T] i32 -> (boxes [B,T,k,9], nms_boxes [B,T,k,7], labels [B,T,k] i32); rows past
    cnt are zero (md_cp_decode_selected)"""
    B, T, k = idx.shape
    dev = head.device
    boxes = torch.empty((B, T, k, 9), dtype=torch.float32, device=dev)
    nms_boxes = torch.empty((B, T, k, 7), dtype=torch.float32, device=dev)
    labels = torch.empty((B, T, k), dtype=torch.int32, device=dev)
    _lib.call("md_cp_decode_selected", [head, idx, cnt, boxes, nms_boxes, labels], extra=at)
    return boxes, nms_boxes, labels


def cp_pack(boxes, sel_scores, labels, keep_idx, num, cnt, at):
    """-> (dets [B, T max_per_task, 11] f32, count [B] i32): per task the first min(num, cnt, max_per_task) kept rows whose score is
    > 0, tasks in order, label + class_base (md_cp_pack = graphs.merge_center_tasks on the per-task outputs)"""
    B, T, _ = sel_scores.shape
    dets = torch.empty((B, T * int(at.max_per_task), 11), dtype=torch.float32, device=boxes.device)
    count = torch.empty((B,), dtype=torch.int32, device=boxes.device)
    _lib.call("md_cp_pack", [boxes, sel_scores, labels, keep_idx, num, cnt, dets, count], extra=at)
    return dets, count


class CenterHeadPostBatched:
    """CenterHead.predict + post_processing (center_head.py:273-463) and the task merge of tools_ms/eval.py:84-111 for every task and
    every sample of the batch, seven launches and no host read: cp_scores over every cell -> one segmented top-k (B T segments,
    nms_pre_max_size each, the masked cells' -1 excluded) -> cp_decode_selected on the selected cells only -> nms_rotated (the
    boxes_iou_nms_cpu rule, count-aware, quota nms_post_max_size: three launches) -> cp_pack.  The result equals CenterHeadPost per
    task + graphs.merge_center_tasks bit for bit."""

    def __init__(self, task_offsets, num_classes, test_cfg):
        self.cfg = test_cfg
        self.at = cp_head_attrs(task_offsets, num_classes, test_cfg)
        self.T = len(num_classes)
        self.pre, self.post = int(test_cfg["nms"]["nms_pre_max_size"]), int(test_cfg["nms"]["nms_post_max_size"])
        self.iou_thr = float(test_cfg["nms"]["nms_iou_threshold"])
        self._segments = {}

    def segments(self, B, n, device):
        """the [B T + 1] int32 table 0, n, 2 n, ... of the top-k: a device constant per batch shape, built on first use"""
        key = (int(B), int(n), str(device))
        if key not in self._segments:
            self._segments[key] = torch.arange(0, (B * self.T + 1) * n, n, dtype=torch.int32, device=device)
        return self._segments[key]

    def __call__(self, head, return_aux=False):
        """head [B,H,W,C] bf16 -> (dets [B, T nms_post_max_size, 11] f32, count [B] i32); rows past count are zero"""
        B, H, W, _ = head.shape
        n, T = H * W, self.T
        scores = cp_scores(head, self.at)
        k = min(self.pre, n)
        vals, idx, cnt = topk_segmented(scores, self.segments(B, n, head.device), k, min_score=-1.0, max_segment=n)
        vals, idx, cnt = vals.view(B, T, k), idx.view(B, T, k), cnt.view(B, T)
        boxes, nms_boxes, labels = cp_decode_selected(head, idx, cnt, self.at)
        keep, num = nms_rotated(nms_boxes.view(B * T, k, 7), self.iou_thr, NMS_ROT_CPU, count=cnt, max_output=self.post)
        dets, count = cp_pack(boxes, vals, labels, keep.view(B, T, k), num.view(B, T), cnt, self.at)
        if return_aux:
            return (dets, count), dict(scores=scores, topk_values=vals, topk_idx=idx, topk_cnt=cnt, boxes=boxes, nms_boxes=nms_boxes,
                                       labels=labels, keep_idx=keep.view(B, T, k), num=num.view(B, T))
        return dets, count


# ----------------------------------------------------------------------------- PointPillars host post-process
def _just_below(x):
    """Largest float32 strictly below x: `score >= x` (predict.py:30) expressed as `score > just_below(x)`."""
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def standup_boxes(boxes):
    """Rotated BEV boxes [N,5] (x,y,dx,dy,r) or [N,7] -> standup boxes [N,4] (predict.py:61-78)."""
    b = _f32c(boxes)
    out = torch.empty((b.shape[0], 4), dtype=torch.float32, device=b.device)
    _lib.call("md_standup_boxes", [b, out])
    return out


def pp_get_selected_data(total_scores, box_preds, anchors_mask, cfg):
    """Mirror of PointPillarsNet.get_selected_data (pointpillars/src/pointpillars.py:753-765) followed by the host
    post-process _get_selected_data (pointpillars/src/predict.py:43-98) for one sample, on device:
    class max / argmax, anchor-mask -> -1, top_k(nms_pre_max_size), score threshold, standup boxes, NMS on the
    standup boxes (nms_jit convention: the reference's ops.NMSWithMask arithmetic is not in the repository),
    first nms_post_max_size survivors.  Returns (boxes[K,7], scores[K], labels[K], count)."""
    top_scores, top_labels = total_scores.max(-1)
    top_scores = torch.where(anchors_mask, top_scores, torch.full_like(top_scores, -1.0))
    k = min(int(cfg["nms_pre_max_size"]), top_scores.numel())
    vals, idx, cnt = topk_segmented(top_scores, torch.tensor([0, top_scores.numel()], dtype=torch.int32, device=top_scores.device),
                                    k, min_score=_just_below(cfg["nms_score_threshold"]) if cfg["nms_score_threshold"] > 0 else None,
                                    max_segment=top_scores.numel())
    sel = gather_rows(_f32c(box_preds).unsqueeze(0), idx, cnt)[0]      # [k,7], zero rows past cnt
    st = standup_boxes(sel)
    mask, kidx, num = nms_aligned(st.unsqueeze(0), float(cfg["nms_iou_threshold"]), 0.0, NMS_MODE_JIT, count=cnt,
                                  max_output=int(cfg["nms_post_max_size"]))
    n = num[0]
    ki = kidx[0].long()
    return sel[ki], vals[0][ki], top_labels[idx[0].long()][ki], n


class _PPHeadAttrs(ctypes.Structure):
    _fields_ = [("off_cls", ctypes.c_int32), ("off_box", ctypes.c_int32), ("off_dir", ctypes.c_int32), ("num_anchors", ctypes.c_int32),
                ("num_classes", ctypes.c_int32), ("score_mode", ctypes.c_int32), ("self_train", ctypes.c_int32)]


def pp_scores(head, off_cls, num_anchors, num_classes, mask=None):
    """head [B,H,W,C] bf16 (the merged head tensor), mask [B,N] bool / uint8 or None -> (scores [B,N] f32, labels [B,N] i32),
    N = H W num_anchors: per anchor the maximum of the class sigmoids and the first class that attains it, -1 where the mask is 0
    (md_pp_scores, include/minddet_hip_pp.h)."""
    B, H, W, _ = head.shape
    n = H * W * int(num_anchors)
    scores = torch.empty((B, n), dtype=torch.float32, device=head.device)
    labels = torch.empty((B, n), dtype=torch.int32, device=head.device)
    if mask is not None:
        mask = mask.to(device=head.device, dtype=torch.uint8).reshape(B, n).contiguous()
    _lib.call("md_pp_scores", [head, mask, scores, labels], extra=_PPHeadAttrs(int(off_cls), 0, -1, int(num_anchors), int(num_classes), 0, 1))
    return scores, labels


def pp_decode_selected(head, anchors, idx, cnt, sel_scores, labels, off_box, off_dir, num_anchors, self_train=True, with_boxes=False):
    """The selected anchors' boxes (md_pp_decode_selected): idx [B,k] i32, cnt [B] i32, sel_scores [B,k] f32 from the top-k, labels
    [B,N] i32 from pp_scores -> (dets [B,k,9] = x, y, z, w, l, h, rot, score, label; standup [B,k,4]; dir_labels [B,k] i32
    [, boxes [B,k,7] before the direction fix]); rows past cnt are zero.  off_dir None / -1: no direction classifier."""
    B, k = idx.shape
    dev = head.device
    dets = torch.empty((B, k, 9), dtype=torch.float32, device=dev)
    standup = torch.empty((B, k, 4), dtype=torch.float32, device=dev)
    dirs = torch.empty((B, k), dtype=torch.int32, device=dev)
    boxes = torch.empty((B, k, 7), dtype=torch.float32, device=dev) if with_boxes else None
    at = _PPHeadAttrs(0, int(off_box), -1 if off_dir is None else int(off_dir), int(num_anchors), 1, 0, int(bool(self_train)))
    _lib.call("md_pp_decode_selected", [head, _f32c(anchors).reshape(-1, 7), idx, cnt, sel_scores, labels, dets, standup, dirs, boxes],
              extra=at)
    return (dets, standup, dirs, boxes) if with_boxes else (dets, standup, dirs)


class PPHeadPost:
    """Post-processing of the anchor-based PointPillars head for a whole batch, five launches and no host read:
    PointPillarsNet.post_processing (pointpillars/src/pointpillars.py:767-800) + _get_selected_data (predict.py:43-98) + the
    direction fix (predict.py:222-236).  pp_scores over every anchor -> one segmented top-k (nms_pre_max_size per sample, score
    threshold as `>=`) -> pp_decode_selected on the selected anchors only -> NMS on the standup boxes (nms_jit convention, as
    pp_get_selected_data) -> the first nms_post_max_size survivors.
    cfg: num_anchors, num_classes, off_cls, off_box, off_dir (None: no direction classifier), nms_pre_max_size, nms_post_max_size,
    nms_score_threshold, nms_iou_threshold [, use_self_train (default True; False is not built)]."""

    def __init__(self, cfg):
        self.cfg = dict(cfg)
        c = self.cfg
        self.A, self.K = int(c["num_anchors"]), int(c["num_classes"])
        self.off_cls, self.off_box, self.off_dir = int(c["off_cls"]), int(c["off_box"]), c.get("off_dir")
        self.pre, self.post = int(c["nms_pre_max_size"]), int(c["nms_post_max_size"])
        self.score_thr, self.iou_thr = float(c["nms_score_threshold"]), float(c["nms_iou_threshold"])
        self.self_train = bool(c.get("use_self_train", True))
        if not self.self_train:
            raise ValueError("PPHeadPost: use_self_train=False (the limit_period direction form, pointpillars.py:637-649) is not built")

    def __call__(self, head, anchors, mask=None, segments=None, return_aux=False):
        """head [B,H,W,C] bf16, anchors [N,7] f32, mask [B,N] or None -> (dets [B, nms_post_max_size, 9] f32, count [B] i32);
        rows past count are zero.  segments: the [B + 1] int32 table 0, N, 2 N, ... (built when not given)."""
        B, H, W, _ = head.shape
        n = H * W * self.A
        dev = head.device
        scores, labels = pp_scores(head, self.off_cls, self.A, self.K, mask)
        if segments is None:
            segments = torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=dev)
        k = min(self.pre, n)
        vals, idx, cnt = topk_segmented(scores, segments, k, min_score=_just_below(self.score_thr) if self.score_thr > 0 else None,
                                        max_segment=n)
        out = pp_decode_selected(head, anchors, idx, cnt, vals, labels, self.off_box, self.off_dir, self.A, with_boxes=return_aux)
        sel, standup, dirs = out[:3]
        keep_mask, kidx, num = nms_aligned(standup, self.iou_thr, 0.0, NMS_MODE_JIT, count=cnt, max_output=self.post)
        ki = kidx[:, :self.post]
        if k < self.post:
            ki = torch.nn.functional.pad(ki, (0, self.post - k))
        dets = gather_rows(sel, ki.contiguous(), num)
        if return_aux:
            return (dets, num), dict(scores=scores, labels=labels, topk_values=vals, topk_idx=idx, topk_cnt=cnt, selected=sel,
                                     standup=standup, dir_labels=dirs, boxes=out[3], keep_mask=keep_mask, keep_idx=kidx)
        return dets, num


# ----------------------------------------------------------------------------- CenterNet post-process (post_process.py)
class _SoftNmsAttrs(ctypes.Structure):
    _fields_ = [("sigma", ctypes.c_float), ("Nt", ctypes.c_float), ("threshold", ctypes.c_float), ("method", ctypes.c_int32)]


def soft_nms(boxes, scores, count=None, sigma=0.5, Nt=0.5, threshold=0.001, method=2):
    """boxes [L,N,4] / [N,4], scores [L,N] / [N] -> (scores_out, order, num). See md_soft_nms."""
    b, s = _f32c(boxes), _f32c(scores)
    batched = b.dim() == 3
    L, n = (b.shape[0], b.shape[1]) if batched else (1, b.shape[0])
    so = torch.empty((L, n), dtype=torch.float32, device=b.device)
    order = torch.empty((L, n), dtype=torch.int32, device=b.device)
    num = torch.empty((L,), dtype=torch.int32, device=b.device)
    _lib.call("md_soft_nms", [b.view(L, n, 4), s.view(L, n), count, so, order, num], extra=_SoftNmsAttrs(sigma, Nt, threshold, method))
    return (so, order, num) if batched else (so[0], order[0], num)


def get_affine_transform(center, scale, output_size, inv=True):
    """centernet/src/image.py (get_affine_transform with rot = 0): the 2x3 matrix cv2.getAffineTransform returns for
    the three reference points, solved here in float64 (cv2 is not a dependency)."""
    scale = np.array([scale, scale], np.float32) if np.isscalar(scale) else np.asarray(scale, np.float32)
    src_w, dst_w, dst_h = scale[0], output_size[0], output_size[1]
    center = np.asarray(center, np.float32)
    src = np.zeros((3, 2), np.float32)
    dst = np.zeros((3, 2), np.float32)
    src[0] = center
    src[1] = center + np.array([0, src_w * -0.5], np.float32)
    dst[0] = [dst_w * 0.5, dst_h * 0.5]
    dst[1] = np.array([dst_w * 0.5, dst_h * 0.5], np.float32) + np.array([0, dst_w * -0.5], np.float32)
    for p in (src, dst):
        d = p[0] - p[1]
        p[2] = p[1] + np.array([-d[1], d[0]], np.float32)
    a, b = (dst, src) if inv else (src, dst)
    A = np.concatenate([a.astype(np.float64), np.ones((3, 1))], 1)
    return np.linalg.solve(A, b.astype(np.float64)).T  # [2,3]


def centernet_post_process(dets, c, s, out_hw, scale, num_classes, soft=True, max_per_image=100):
    """Mirror of post_process + merge_outputs (centernet/src/post_process.py:10-61) for one image, on device.
    dets [K,6] (x1,y1,x2,y2,score,cls) in feature-map units -> rows surviving the per-class (soft-)NMS and the
    global top-max_per_image cut, in image coordinates: (boxes [M,4], scores [M], classes [M])."""
    t = torch.from_numpy(get_affine_transform(c, s, (out_hw[1], out_hw[0]))).to(dets.device)
    d = dets.to(torch.float64)
    xy1 = (d[:, 0:2] @ t[:, :2].T + t[:, 2]).to(torch.float32) / scale
    xy2 = (d[:, 2:4] @ t[:, :2].T + t[:, 2]).to(torch.float32) / scale
    boxes = torch.cat([xy1, xy2], 1).contiguous()
    scores, cls = dets[:, 4].contiguous(), dets[:, 5].to(torch.int32)
    K = boxes.shape[0]
    if soft:
        # per-class lists: class-major padding [C, K]
        lists_b = torch.zeros((num_classes, K, 4), dtype=torch.float32, device=dets.device)
        lists_s = torch.zeros((num_classes, K), dtype=torch.float32, device=dets.device)
        cnt = torch.zeros((num_classes,), dtype=torch.int32, device=dets.device)
        pos = torch.zeros((K,), dtype=torch.long, device=dets.device)
        for j in range(num_classes):  # classes == j split (post_process.py:19-27); tiny host loop over <= 80 classes
            idx = torch.nonzero(cls == j).flatten()
            m = idx.numel()
            if m:
                lists_b[j, :m], lists_s[j, :m], cnt[j] = boxes[idx], scores[idx], m
                pos[idx] = torch.arange(m, device=dets.device)
        so, _, _ = soft_nms(lists_b, lists_s, cnt)
        scores = so[cls.long(), pos]
        alive = scores > 0
    else:
        alive = torch.ones_like(scores, dtype=torch.bool)
    s_alive = scores[alive]
    if s_alive.numel() > max_per_image:  # np.partition threshold, ties may exceed max_per_image (post_process.py:54-60)
        thresh = torch.sort(s_alive)[0][s_alive.numel() - max_per_image]
        alive = alive & (scores >= thresh)
    return boxes[alive], scores[alive], cls[alive]


class _RotIouAttrs(ctypes.Structure):
    _fields_ = [("criterion", ctypes.c_int32)]


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1):
    """pointpillars/eval_gpu/rotate_iou.py:305-340: [N,5] x [K,5] (cx,cy,dx,dy,angle) -> [N,K]."""
    b, q = _f32c(boxes), _f32c(query_boxes)
    out = torch.empty((b.shape[0], q.shape[0]), dtype=torch.float32, device=b.device)
    _lib.call("md_rotate_iou_eval", [b, q, out], extra=_RotIouAttrs(int(criterion)))
    return out


# ----------------------------------------------------------------------------- YOLOv5 Detect decode
class _YoloAttrs(ctypes.Structure):
    _fields_ = [("num_classes", ctypes.c_int32), ("num_anchors", ctypes.c_int32), ("stride", ctypes.c_float),
                ("anchors", ctypes.c_float * 6), ("conf_thres", ctypes.c_float), ("out_offset", ctypes.c_int32),
                ("out_total", ctypes.c_int32)]


def yolo_decode(head, boxes, scores, labels, num_classes, num_anchors, stride, anchors, conf_thres, out_offset, out_total):
    at = _YoloAttrs(int(num_classes), int(num_anchors), float(stride))
    for i, v in enumerate(anchors):
        at.anchors[i] = float(v)
    at.conf_thres, at.out_offset, at.out_total = float(conf_thres), int(out_offset), int(out_total)
    _lib.call("md_yolo_decode", [head, boxes, scores, labels], extra=at)


def assign_targets(anchors, gt_boxes, gt_classes, matched_thr, unmatched_thr, anchors_mask=None):
    """create_target_np (pointpillars/src/core/target_assigner.py:29-166; TargetAssigner.assign :196-224) on the device:
    -> (labels [A] i32, bbox_targets [A,7] f32, bbox_outside_weights [A] f32, gt_ids [A] i32).  Thresholds: float or [A];
    gt_boxes None or [0,7]: a scene without ground truth."""
    a = _f32c(anchors).reshape(-1, 7)
    dev, A = a.device, a.shape[0]
    g = None if gt_boxes is None else _f32c(gt_boxes).reshape(-1, 7)
    G = 0 if g is None else g.shape[0]
    cls = (torch.ones((G,), dtype=torch.int32, device=dev) if gt_classes is None
           else gt_classes.to(device=dev, dtype=torch.int32).contiguous())

    def thr(v):
        return (torch.full((A,), float(v), dtype=torch.float32, device=dev) if not torch.is_tensor(v) else _f32c(v).reshape(-1))

    mt, ut = thr(matched_thr), thr(unmatched_thr)
    mask = None if anchors_mask is None else anchors_mask.to(device=dev, dtype=torch.uint8).contiguous()
    labels = torch.empty((A,), dtype=torch.int32, device=dev)
    targets = torch.empty((A, 7), dtype=torch.float32, device=dev)
    weights = torch.empty((A,), dtype=torch.float32, device=dev)
    gt_ids = torch.empty((A,), dtype=torch.int32, device=dev)
    _lib.call("md_assign_targets", [a, g if G else None, cls if G else None, mt, ut, mask, labels, targets, weights, gt_ids])
    return labels, targets, weights, gt_ids


def mask_select(logits, dets, num_classes):
    """[R,S,S,Cpad] bf16 mask logits + [R,6] detections -> [R,S,S] f32 sigmoid of each detection's own class channel."""
    r, sz = logits.shape[0], logits.shape[1]
    out = torch.empty((r, sz, sz), dtype=torch.float32, device=logits.device)
    _lib.call("md_mask_select", [logits, _f32c(dets).reshape(-1, 6), out], extra=ctypes.c_int32(int(num_classes)))
    return out


class _PasteAttrs(ctypes.Structure):
    _fields_ = [("img_h", ctypes.c_int32), ("img_w", ctypes.c_int32), ("threshold", ctypes.c_float), ("bits", ctypes.c_int32)]


def paste_masks(masks, dets, img_hw, threshold=0.5, bits=True):
    """[B,D,S,S] f32 mask probabilities + [B,D,6] detections -> image-resolution masks (md_paste_masks): bits=True ->
    [B,D,H,ceil(W/32)] int32 words (bit j of word k = pixel 32 k + j), else [B,D,H,W] uint8 (0 / 1)."""
    B, D, S = masks.shape[0], masks.shape[1], masks.shape[2]
    H, W = int(img_hw[0]), int(img_hw[1])
    if bits:
        out = torch.empty((B * D, H, (W + 31) // 32), dtype=torch.int32, device=masks.device)
    else:
        out = torch.empty((B * D, H, W), dtype=torch.uint8, device=masks.device)
    _lib.call("md_paste_masks", [_f32c(masks).reshape(B * D, S, S), _f32c(dets).reshape(B * D, 6), out],
              extra=_PasteAttrs(H, W, float(threshold), int(bool(bits))))
    return out.view(B, D, H, out.shape[2])


def unpack_mask_bits(words, width):
    """[..., H, ceil(W/32)] int32 bit masks -> [..., H, W] uint8 (host-side helper for tests / result export)."""
    w = words.to(torch.int64) & 0xffffffff
    sh = torch.arange(32, device=words.device, dtype=torch.int64)
    return ((w.unsqueeze(-1) >> sh) & 1).reshape(*words.shape[:-1], -1)[..., :width].to(torch.uint8)


def dets_to_rois(dets):
    """[B,D,6] detections -> [B*D,5] RoIs (batch index, x1, y1, x2, y2) for the mask head (layout plumbing)."""
    B, D = dets.shape[0], dets.shape[1]
    b = torch.arange(B, dtype=torch.float32, device=dets.device).view(B, 1, 1).expand(B, D, 1)
    return torch.cat([b, dets[..., :4]], -1).reshape(B * D, 5).contiguous()


class _Yolo8Attrs(ctypes.Structure):
    _fields_ = [("num_classes", ctypes.c_int32), ("reg_max", ctypes.c_int32), ("stride", ctypes.c_float), ("conf_thres", ctypes.c_float),
                ("out_offset", ctypes.c_int32), ("out_total", ctypes.c_int32)]


def yolov8_decode(head, boxes, scores, labels, num_classes, reg_max, stride, conf_thres, out_offset, out_total):
    _lib.call("md_yolov8_decode", [head, boxes, scores, labels],
              extra=_Yolo8Attrs(int(num_classes), int(reg_max), float(stride), float(conf_thres), int(out_offset), int(out_total)))


# ----------------------------------------------------------------------------- point-cloud front end (csrc/pillars.hip)
class _VoxelizeAttrs(ctypes.Structure):
    _fields_ = [("voxel_size", ctypes.c_float * 3), ("range", ctypes.c_float * 6), ("max_points", ctypes.c_int32),
                ("max_voxels", ctypes.c_int32)]


class _PillarEncodeAttrs(ctypes.Structure):
    _fields_ = [("vx", ctypes.c_float), ("vy", ctypes.c_float), ("x_offset", ctypes.c_float), ("y_offset", ctypes.c_float),
                ("with_distance", ctypes.c_int32), ("virtual_points", ctypes.c_int32)]


def voxel_grid(voxel_size, pc_range):
    """cells per axis (x, y, z) as the reference computes them: round((max - min) / voxel_size) in fp32 (point_cloud_ops.py:24-27)"""
    vs, r = np.asarray(voxel_size, np.float32), np.asarray(pc_range, np.float32)
    return tuple(int(v) for v in np.round((r[3:] - r[:3]) / vs).astype(np.int32))


def voxelize_workspace_bytes(N, B, cells, max_voxels):
    """bytes of scratch md_voxelize takes for N points, B samples of `cells` cells (include/minddet_hip_points.h)"""
    return _lib.workspace_bytes("md_voxelize", N, B, cells, max_voxels)


def voxelize(points, offsets, voxel_size, pc_range, max_points, max_voxels):
    """points [N, F] f32 (F = 4 or 5; B samples back to back), offsets [B + 1] i32 on the device ->
    (voxels [B, max_voxels, max_points, F] f32, coors [B, max_voxels, 4] i32 (b, z, y, x), num_points [B, max_voxels] i32,
    voxel_num [B] i32): points_to_voxel(reverse_index=True) per sample, bit for bit (md_voxelize; no host round trip)."""
    if points.dim() != 2 or points.shape[1] not in (4, 5):
        raise ValueError(f"voxelize: points are [N, 4] or [N, 5], got {tuple(points.shape)}")
    points = _f32c(points)
    dev, (N, F), B = points.device, points.shape, offsets.numel() - 1
    max_points, max_voxels = int(max_points), int(max_voxels)
    at = _VoxelizeAttrs((ctypes.c_float * 3)(*[float(v) for v in voxel_size]), (ctypes.c_float * 6)(*[float(v) for v in pc_range]),
                        max_points, max_voxels)
    gx, gy, gz = voxel_grid(voxel_size, pc_range)
    voxels = torch.empty((B, max_voxels, max_points, F), dtype=torch.float32, device=dev)
    coors = torch.empty((B, max_voxels, 4), dtype=torch.int32, device=dev)
    num_points = torch.empty((B, max_voxels), dtype=torch.int32, device=dev)
    voxel_num = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = _lib.scratch("md_voxelize", (N, B, gx * gy * gz, max_voxels), dev)
    _lib.call("md_voxelize", [points, offsets, voxels, coors, num_points, voxel_num, ws], extra=at)
    return voxels, coors, num_points, voxel_num


class PackedPFN:
    """The PFN layers as md_pillar_encode takes them: per layer the Dense weight with the BatchNorm folded in (fp32)."""

    def __init__(self, w1, b1, w2=None, b2=None):
        self.w1, self.b1, self.w2, self.b2 = w1, b1, w2, b2

    def to(self, device):
        self.w1, self.b1 = self.w1.to(device), self.b1.to(device)
        if self.w2 is not None:
            self.w2, self.b2 = self.w2.to(device), self.b2.to(device)
        return self


def pack_pfn(layers):
    """layers: one (weight [units, in] f32, (gamma, beta, mean, var, eps)) per PFN layer -> PackedPFN.  The fold, in fp32:
    scale = gamma / sqrt(var + eps); w = weight * scale per output row; b = beta - mean * scale.  One layer [64, F + 5] or two layers
    [32, F + 5] and [64, 64]; anything else raises ValueError."""
    if len(layers) not in (1, 2):
        raise ValueError(f"pack_pfn: one or two PFN layers are supported, got {len(layers)}")
    out = []
    for weight, (gamma, beta, mean, var, eps) in layers:
        weight = torch.as_tensor(weight, dtype=torch.float32)
        scale = torch.as_tensor(gamma, dtype=torch.float32) / torch.sqrt(torch.as_tensor(var, dtype=torch.float32) + float(eps))
        out += [(weight * scale[:, None]).contiguous(), (torch.as_tensor(beta, dtype=torch.float32)
                                                        - torch.as_tensor(mean, dtype=torch.float32) * scale).contiguous()]
    want = [(64,)] if len(layers) == 1 else [(32,), (64, 64)]
    if out[0].shape[0] != want[0][0] or out[0].shape[1] not in (9, 10) or (len(layers) == 2 and tuple(out[2].shape) != want[1]):
        raise ValueError(f"pack_pfn: supported are num_filters (64,) and (64, 64) on 4 or 5 point features, got weights "
                         f"{[tuple(w.shape) for w in out[0::2]]}")
    return PackedPFN(*out)


def pillar_encode(voxels, num_points, coors, voxel_num, pfn, hw, vx, vy, x_offset, y_offset, out=None):
    """PillarFeatureNet + PointPillarsScatter (md_pillar_encode): the outputs of voxelize and a PackedPFN -> the pseudo-image
    [B, H, W, 64] bf16 (NHWC), zero where no pillar is."""
    B = voxels.shape[0]
    H, W = int(hw[0]), int(hw[1])
    canvas = out if out is not None else torch.empty((B, H, W, 64), dtype=torch.bfloat16, device=voxels.device)
    at = _PillarEncodeAttrs(float(vx), float(vy), float(x_offset), float(y_offset), 0, 0)
    _lib.call("md_pillar_encode", [voxels, num_points, coors, voxel_num, pfn.w1, pfn.b1, pfn.w2, pfn.b2, canvas], extra=at)
    return canvas


# ----------------------------------------------------------------------------- KITTI PointPillars front end (csrc/ppreader.hip)
class _PPPillarEncodeAttrs(ctypes.Structure):
    _fields_ = [("vx", ctypes.c_float), ("vy", ctypes.c_float), ("vz", ctypes.c_float), ("x_offset", ctypes.c_float),
                ("y_offset", ctypes.c_float), ("z_offset", ctypes.c_float), ("with_distance", ctypes.c_int32), ("reserved0", ctypes.c_int32)]


class PackedPPReader:
    """The KITTI reader's one PFN layer as md_pp_pillar_encode takes it: the RAW Dense weight [64, K] (the op rounds it to fp16 as the
    reference's to_float(float16) does, so the BatchNorm must not be folded into it) and the BatchNorm as scale, shift [64] in fp32."""

    def __init__(self, w, scale, shift):
        self.w, self.scale, self.shift = w, scale, shift

    def to(self, device):
        self.w, self.scale, self.shift = self.w.to(device), self.scale.to(device), self.shift.to(device)
        return self


def pack_pp_pfn(layers):
    """layers: [(weight [64, K] f32, (gamma, beta, mean, var, eps))], K = 10 or 11 -> PackedPPReader.  In fp32:
    scale = gamma / sqrt(var + eps), shift = beta - mean * scale; the weight is kept as it is."""
    if len(layers) != 1:
        raise ValueError(f"pack_pp_pfn: the KITTI reader is built with one PFN layer, got {len(layers)}")
    weight, (gamma, beta, mean, var, eps) = layers[0]
    weight = torch.as_tensor(weight, dtype=torch.float32).contiguous()
    if weight.dim() != 2 or weight.shape[0] != 64 or weight.shape[1] not in (10, 11):
        raise ValueError(f"pack_pp_pfn: the Dense weight is [64, 10] or [64, 11] (with_distance), got {tuple(weight.shape)}")
    scale = torch.as_tensor(gamma, dtype=torch.float32) / torch.sqrt(torch.as_tensor(var, dtype=torch.float32) + float(eps))
    shift = torch.as_tensor(beta, dtype=torch.float32) - torch.as_tensor(mean, dtype=torch.float32) * scale
    return PackedPPReader(weight, scale.contiguous(), shift.contiguous())


def pp_pillar_encode(voxels, num_points, coors, voxel_num, pfn, hw, voxel_size, offsets, out=None):
    """The KITTI model's PillarFeatureNet + PointPillarsScatter (md_pp_pillar_encode): the outputs of voxelize ([.., 4] points) and a
    PackedPPReader -> the pseudo-image [B, H, W, 64] bf16 (NHWC), zero where no pillar is.  voxel_size = (vx, vy, vz), offsets =
    (x, y, z): the centre of cell 0 per axis.  with_distance follows the weight's width."""
    B = voxels.shape[0]
    H, W = int(hw[0]), int(hw[1])
    canvas = out if out is not None else torch.empty((B, H, W, 64), dtype=torch.bfloat16, device=voxels.device)
    at = _PPPillarEncodeAttrs(*[float(v) for v in voxel_size[:3]], *[float(v) for v in offsets[:3]], int(pfn.w.shape[1] == 11), 0)
    _lib.call("md_pp_pillar_encode", [voxels, num_points, coors, voxel_num, pfn.w, pfn.scale, pfn.shift, canvas], extra=at)
    return canvas


def anchors_mask_batched(coors, voxel_num, grid_size_xy, anchors_bv, voxel_size, pc_range, area_threshold, with_area=False):
    """preprocess.py:211-225 for the batch (md_pp_anchor_mask): coors [B, MV, 4] i32 (b, z, y, x) and voxel_num [B] i32 as voxelize
    leaves them -> mask [B, N] uint8 (, area [B, N] f32): row b is anchors_mask(coors[b, :voxel_num[b], 1:]) bit for bit, with
    voxel_num read on the device."""
    at = _AnchorMaskAttrs(int(grid_size_xy[0]), int(grid_size_xy[1]), float(voxel_size[0]), float(voxel_size[1]),
                          float(pc_range[0]), float(pc_range[1]), float(area_threshold))
    bv = _f32c(anchors_bv)
    B, dev = coors.shape[0], bv.device
    mask = torch.empty((B, bv.shape[0]), dtype=torch.uint8, device=dev)
    area = torch.empty((B, bv.shape[0]), dtype=torch.float32, device=dev) if with_area else None
    ws = _lib.scratch("md_pp_anchor_mask", (B, at.grid_x, at.grid_y), dev)
    _lib.call("md_pp_anchor_mask", [coors, voxel_num, bv, mask, area, ws], extra=at)
    return (mask, area) if with_area else mask


# ----------------------------------------------------------------------------- KITTI training augmentation (csrc/pcaug.hip)
PCAUG_MAX_BOXES, PCAUG_MAX_TRIES = 256, 128     # MD_PCAUG_MAX_BOXES, MD_PCAUG_MAX_TRIES


class _PCBoxesAttrs(ctypes.Structure):
    _fields_ = [("bv_range", ctypes.c_float * 4)]


def _i32c(t, dev):
    return t.to(device=dev, dtype=torch.int32).contiguous()


def _f64c(t, dev):
    return t.to(device=dev, dtype=torch.float64).contiguous()


def pc_noise_per_object(gt_boxes, gt_count, valid, loc_noises, rot_noises, grot_noises=None):
    """noise_per_object without groups (pointpillars/src/core/preprocess.py:560-668) for a batch on the device
    (md_pc_noise_per_object, include/minddet_hip_pcaug.h): gt_boxes [B,G,7] f32, gt_count [B], valid [B,G], the draws loc_noises
    [B,G,T,3], rot_noises [B,G,T] and grot_noises [B,G,T] or None (None: noise_per_box, no per-object global rotation) in float64
    -> (selected [B,G] i32, obj_transform [B,G,4] f64, boxes_out [B,G,7] f32)."""
    g = _f32c(gt_boxes)
    if g.dim() != 3 or g.shape[2] != 7:
        raise ValueError(f"pc_noise_per_object: gt_boxes are [B, G, 7] (boxes wider than 7 are not built), got {tuple(g.shape)}")
    dev, (B, G) = g.device, g.shape[:2]
    if G > PCAUG_MAX_BOXES or not 1 <= rot_noises.shape[-1] <= PCAUG_MAX_TRIES:
        raise ValueError(f"pc_noise_per_object: at most {PCAUG_MAX_BOXES} boxes and 1 .. {PCAUG_MAX_TRIES} tries per sample")
    selected = torch.empty((B, G), dtype=torch.int32, device=dev)
    tf = torch.empty((B, G, 4), dtype=torch.float64, device=dev)
    out = torch.empty((B, G, 7), dtype=torch.float32, device=dev)
    _lib.call("md_pc_noise_per_object", [g, _i32c(gt_count, dev), valid.to(device=dev, dtype=torch.uint8).contiguous(), _f64c(loc_noises, dev),
                                         _f64c(rot_noises, dev), None if grot_noises is None else _f64c(grot_noises, dev), selected, tf, out])
    return selected, tf, out


def pc_augment_points_workspace_bytes(N, B, G, R):
    """bytes of scratch md_pc_augment_points takes (include/minddet_hip_pcaug.h)"""
    return _lib.workspace_bytes("md_pc_augment_points", N, B, G, R)


def pc_augment_points(points, offsets, obj_boxes, gt_count, valid, obj_transform, glob, remove_boxes=None, remove_count=None,
                      remove_from=None, workspace=True):
    """remove_points_in_boxes + points_transform_ + the point side of the four global steps + a stable compaction
    (md_pc_augment_points): points [N,4] f32 with offsets [B+1] i32 as voxelize takes them, obj_boxes [B,G,7] f32 (BEFORE the noise),
    obj_transform [B,G,4] f64 of pc_noise_per_object, glob [B,6] f64 (flip, rotation, scale, tx, ty, tz), optionally remove_boxes
    [B,R,7] with remove_count [B] and remove_from [B] -> (points_out [N,4] f32, offsets_out [B+1] i32, owner [N] i32).
    workspace=False leaves the scratch to the library's per-stream pool."""
    if points.dim() != 2 or points.shape[1] != 4:
        raise ValueError(f"pc_augment_points: points are [N, 4] (without_reflectivity is not built), got {tuple(points.shape)}")
    points, g = _f32c(points), _f32c(obj_boxes)
    dev, N, B, G = points.device, points.shape[0], g.shape[0], g.shape[1]
    rem = [None, None, None]
    if remove_boxes is not None:
        if remove_count is None or remove_from is None:
            raise ValueError("pc_augment_points: remove_boxes come with remove_count and remove_from")
        rem = [_f32c(remove_boxes), _i32c(remove_count, dev), _i32c(remove_from, dev)]
    R = 0 if rem[0] is None else rem[0].shape[1]
    out = torch.empty((N, 4), dtype=torch.float32, device=dev)
    offsets_out = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    owner = torch.empty((N,), dtype=torch.int32, device=dev)
    ops = [points, _i32c(offsets, dev), g, _i32c(gt_count, dev), valid.to(device=dev, dtype=torch.uint8).contiguous(),
           _f64c(obj_transform, dev), *rem, _f64c(glob, dev), out, offsets_out, owner]
    if workspace:
        ops.append(_lib.scratch("md_pc_augment_points", (N, B, G, R), dev))
    _lib.call("md_pc_augment_points", ops)
    return out, offsets_out, owner


def pc_augment_boxes(boxes, gt_count, valid, classes, glob, bv_range):
    """the box side of the four global steps, filter_gt_box_outside_range, limit_period and the gt_boxes_mask selection
    (md_pc_augment_boxes): boxes [B,G,7] f32 (pc_noise_per_object's boxes_out), classes [B,G], glob [B,6] f64, bv_range (x min, y min,
    x max, y max) -> (gt_boxes [B,G,7] f32 and gt_classes [B,G] i32, the kept rows in front and zeros behind, out_count [B] i32)."""
    g = _f32c(boxes)
    if g.dim() != 3 or g.shape[2] != 7:
        raise ValueError(f"pc_augment_boxes: boxes are [B, G, 7], got {tuple(g.shape)}")
    dev, (B, G) = g.device, g.shape[:2]
    at = _PCBoxesAttrs((ctypes.c_float * 4)(*[float(v) for v in bv_range]))
    out = torch.empty((B, G, 7), dtype=torch.float32, device=dev)
    cls = torch.empty((B, G), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call("md_pc_augment_boxes", [g, _i32c(gt_count, dev), valid.to(device=dev, dtype=torch.uint8).contiguous(), _i32c(classes, dev),
                                      _f64c(glob, dev), out, cls, count], extra=at)
    return out, cls, count


_PCAUG_REFUSED = ("group_ids", "use_group_id", "reference_detections", "remove_environment", "remove_outside_points", "without_reflectivity",
                  "bev_only", "shuffle_points")


class PointCloudAugment:
    """The training branch of prep_pointcloud (pointpillars/src/data/preprocess.py:124-170) on the device, built from the reference's
    keys and defaults (:24-29): gt_rotation_noise, gt_loc_noise_std, global_rotation_noise, global_scaling_noise, global_loc_noise_std,
    global_random_rot_range, plus num_try (100, :144), flip_probability (0.5, core/preprocess.py:686) and bv_range (x min, y min, x max,
    y max of the voxel generator's range, :162).  group_ids, reference_detections, remove_environment, remove_outside_points,
    without_reflectivity, bev_only and shuffle_points are not built: a true value raises ValueError."""

    def __init__(self, bv_range, gt_rotation_noise=(-math.pi / 3, math.pi / 3), gt_loc_noise_std=(1.0, 1.0, 1.0),
                 global_rotation_noise=(-math.pi / 4, math.pi / 4), global_scaling_noise=(0.95, 1.05), global_loc_noise_std=(0.2, 0.2, 0.2),
                 global_random_rot_range=(0.78, 2.35), num_try=100, flip_probability=0.5, **options):
        for k, v in options.items():
            if k not in _PCAUG_REFUSED:
                raise ValueError(f"PointCloudAugment: unknown option {k!r}")
            if v not in (None, False):
                raise ValueError(f"PointCloudAugment: {k} is not built")

        def pair(v):           # a scalar means [-v, v] (core/preprocess.py:572-575, 673-674)
            return (-float(v), float(v)) if not isinstance(v, (list, tuple)) else (float(v[0]), float(v[1]))

        def triple(v):
            return (float(v),) * 3 if not isinstance(v, (list, tuple)) else tuple(float(x) for x in v)

        self.bv_range = tuple(float(v) for v in bv_range)
        self.gt_rotation_noise, self.gt_loc_noise_std = pair(gt_rotation_noise), triple(gt_loc_noise_std)
        self.global_rotation_noise, self.global_scaling_noise = pair(global_rotation_noise), pair(global_scaling_noise)
        self.global_loc_noise_std, self.global_random_rot_range = triple(global_loc_noise_std), pair(global_random_rot_range)
        self.num_try, self.flip_probability = int(num_try), float(flip_probability)
        if len(self.bv_range) != 4 or len(self.gt_loc_noise_std) != 3 or len(self.global_loc_noise_std) != 3:
            raise ValueError("PointCloudAugment: bv_range has 4 values, the noise stds 3")
        if not 1 <= self.num_try <= PCAUG_MAX_TRIES:
            raise ValueError(f"PointCloudAugment: num_try in 1 .. {PCAUG_MAX_TRIES}, got {self.num_try}")
        # enable_grot, core/preprocess.py:576-578
        self.enable_grot = abs(self.global_random_rot_range[0] - self.global_random_rot_range[1]) >= 1e-3

    @classmethod
    def from_config(cls, cfg):
        """cfg.train_cfg["augment"] (the reference's keys) and the voxel generator's range"""
        r = cfg.model["voxel_generator"]["point_cloud_range"]
        return cls((r[0], r[1], r[3], r[4]), **dict(cfg.train_cfg["augment"]))

    def draw(self, gt_boxes, gt_count, generator=None):
        """The random draws of one batch as float64 device tensors, with the reference's distributions: loc [B,G,T,3] normal with
        gt_loc_noise_std, rot [B,G,T] uniform in gt_rotation_noise, grot [B,G,T] uniform in global_random_rot_range shifted per box by
        -atan2(x, y) (core/preprocess.py:584-595; None unless enable_grot), glob [B,6] = (flip with flip_probability, rotation uniform in
        global_rotation_noise, scale uniform in global_scaling_noise, translation normal with global_loc_noise_std x, y and -- as the
        reference does, :800 -- x again for z).  The draws come from torch's generator (`generator`: a torch.Generator of the boxes'
        device, None = the default one), NOT from numpy's random stream: the reference's distributions, not its sequence."""
        g = _f32c(gt_boxes)
        dev, (B, G), T = g.device, g.shape[:2], self.num_try
        f64 = dict(dtype=torch.float64, device=dev, generator=generator)

        def uniform(shape, lo, hi):
            return lo + (hi - lo) * torch.rand(shape, **f64)

        loc = torch.randn((B, G, T, 3), **f64) * torch.tensor(self.gt_loc_noise_std, dtype=torch.float64, device=dev)
        rot = uniform((B, G, T), *self.gt_rotation_noise)
        grot = None
        if self.enable_grot:
            shift = torch.atan2(g[..., 0].double(), g[..., 1].double())[..., None]
            grot = uniform((B, G, T), *self.global_random_rot_range) - shift
        glob = torch.empty((B, 6), dtype=torch.float64, device=dev)
        glob[:, 0] = (torch.rand((B,), **f64) < self.flip_probability).double()
        glob[:, 1] = uniform((B,), *self.global_rotation_noise)
        glob[:, 2] = uniform((B,), *self.global_scaling_noise)
        std = self.global_loc_noise_std
        glob[:, 3:6] = torch.randn((B, 3), **f64) * torch.tensor([std[0], std[1], std[0]], dtype=torch.float64, device=dev)
        return dict(loc=loc, rot=rot, grot=grot, glob=glob)

    def __call__(self, points, offsets, gt_boxes, gt_classes, gt_count, valid=None, sampled=None, draws=None, generator=None):
        """points [N,4] f32, offsets [B+1] i32, gt_boxes [B,G,7] f32, gt_classes [B,G], gt_count [B]; valid [B,G] (None: every row);
        sampled = dict(remove_boxes [B,R,7], remove_count [B], remove_from [B]) when the caller put sampled objects' points in front
        of each sample; draws = the dict of draw() (None: drawn here) -> dict(points, offsets, gt_boxes, gt_classes, gt_count,
        selected, owner), nothing read back."""
        g = _f32c(gt_boxes)
        dev = g.device
        if valid is None:
            valid = torch.ones(g.shape[:2], dtype=torch.uint8, device=dev)
        if draws is None:
            draws = self.draw(g, gt_count, generator)
        if (draws.get("grot") is not None) != self.enable_grot:
            raise ValueError("PointCloudAugment: draws carry grot exactly when global_random_rot_range is an interval")
        selected, tf, moved = pc_noise_per_object(g, gt_count, valid, draws["loc"], draws["rot"], draws.get("grot"))
        s = dict(sampled or {})
        pts, offs, owner = pc_augment_points(points, offsets, g, gt_count, valid, tf, draws["glob"], s.get("remove_boxes"),
                                             s.get("remove_count"), s.get("remove_from"))
        boxes, classes, count = pc_augment_boxes(moved, gt_count, valid, gt_classes, draws["glob"], self.bv_range)
        return dict(points=pts, offsets=offs, gt_boxes=boxes, gt_classes=classes, gt_count=count, selected=selected, owner=owner)


# ----------------------------------------------------------------------------- CenterPoint training input (csrc/cpaug.hip)
CPAUG_MAX_GT, CPAUG_MAX_CAND = 512, 256     # MD_CPAUG_MAX_GT, MD_CPAUG_MAX_CAND


class _CPCountAttrs(ctypes.Structure):
    _fields_ = [("min_points", ctypes.c_int32)]


class _CPBoxesAttrs(ctypes.Structure):
    _fields_ = [("bv_range", ctypes.c_float * 4)]


def _u8c(t, dev):
    return t.to(device=dev, dtype=torch.uint8).contiguous()


def _boxes9(who, t):
    g = _f32c(t)
    if g.dim() != 3 or g.shape[2] != 9:
        raise ValueError(f"{who}: boxes are [B, n, 9] (x, y, z, w, l, h, vx, vy, r), got {tuple(g.shape)}")
    return g


def _points5(who, t):
    if t.dim() != 2 or t.shape[1] != 5:
        raise ValueError(f"{who}: points are [N, 5], got {tuple(t.shape)}")
    return _f32c(t)


def cp_aug_count_points_workspace_bytes(B, G):
    """bytes of scratch md_cp_aug_count_points takes (include/minddet_hip_cpaug.h)"""
    return _lib.workspace_bytes("md_cp_aug_count_points", B, G)


def cp_aug_count_points(points, offsets, gt_boxes, gt_count, min_points=-1, workspace=True):
    """points_count_rbbox + the min_points_in_gt mask (md_cp_aug_count_points, include/minddet_hip_cpaug.h): points [N,5] f32 with
    offsets [B+1] i32 as voxelize takes them, gt_boxes [B,G,9] f32, gt_count [B] -> (counts [B,G] i32, keep [B,G] u8 = g < gt_count and
    (min_points <= 0 or counts >= min_points)).  workspace=False leaves the scratch to the library's per-stream pool."""
    points, g = _points5("cp_aug_count_points", points), _boxes9("cp_aug_count_points", gt_boxes)
    dev, (B, G) = g.device, g.shape[:2]
    counts = torch.empty((B, G), dtype=torch.int32, device=dev)
    keep = torch.empty((B, G), dtype=torch.uint8, device=dev)
    ops = [points, _i32c(offsets, dev), g, _i32c(gt_count, dev), counts, keep]
    if workspace:
        ops.append(_lib.scratch("md_cp_aug_count_points", (B, G), dev))
    _lib.call("md_cp_aug_count_points", ops, extra=_CPCountAttrs(int(min_points)))
    return counts, keep


def cp_aug_select_workspace_bytes(B, G, S):
    """bytes of scratch md_cp_aug_select takes (include/minddet_hip_cpaug.h)"""
    return _lib.workspace_bytes("md_cp_aug_select", B, G, S)


def cp_aug_select(gt_boxes, gt_count, keep, cand_boxes, cand_count, cand_group, workspace=True):
    """the accept step of the ground-truth sampler (md_cp_aug_select): gt_boxes [B,G,9], gt_count [B], keep [B,G] u8 of
    cp_aug_count_points, cand_boxes [B,S,9] in draw order, cand_count [B], cand_group [B,S] i32 (non-decreasing per sample, one value
    per sample_class_v2 call) -> accept [B,S] u8.  A sample whose groups decrease accepts nothing."""
    g, c = _boxes9("cp_aug_select", gt_boxes), _boxes9("cp_aug_select", cand_boxes)
    dev, (B, G), S = g.device, g.shape[:2], c.shape[1]
    accept = torch.empty((B, S), dtype=torch.uint8, device=dev)
    ops = [g, _i32c(gt_count, dev), _u8c(keep, dev), c, _i32c(cand_count, dev), _i32c(cand_group, dev), accept]
    if workspace:
        ops.append(_lib.scratch("md_cp_aug_select", (B, G, S), dev))
    _lib.call("md_cp_aug_select", ops)
    return accept


def cp_aug_points_workspace_bytes(N, Ns, B):
    """bytes of scratch md_cp_aug_points takes (include/minddet_hip_cpaug.h)"""
    return _lib.workspace_bytes("md_cp_aug_points", N, Ns, B)


def cp_aug_points(points, offsets, glob, cand_points=None, cand_offsets=None, cand_boxes=None, accept=None, workspace=True):
    """the accepted candidates' points (each plus its box centre) in front of every sample's scene points, then the point side of
    the two flips, the rotation, the scale and the translation (md_cp_aug_points): points [N,5] f32, offsets [B+1] i32, glob [B,7]
    f64 (flip_a, flip_b, rot, scale, tx, ty, tz); cand_points [Ns,5] f32 in each candidate's frame, cand_offsets [B S + 1] i32,
    cand_boxes [B,S,9], accept [B,S] u8 -- all four or none -> (points_out [N+Ns,5] f32 with zero rows behind the last kept row,
    offsets_out [B+1] i32)."""
    points = _points5("cp_aug_points", points)
    dev, N, B = points.device, points.shape[0], offsets.numel() - 1
    cand = [cand_points, cand_offsets, cand_boxes, accept]
    if any(c is None for c in cand) != all(c is None for c in cand):
        raise ValueError("cp_aug_points: cand_points, cand_offsets, cand_boxes and accept come together")
    Ns = 0
    if cand_points is not None:
        cand = [_points5("cp_aug_points", cand_points.to(dev)), _i32c(cand_offsets, dev), _boxes9("cp_aug_points", cand_boxes), _u8c(accept, dev)]
        Ns = cand[0].shape[0]
    out = torch.empty((N + Ns, 5), dtype=torch.float32, device=dev)
    offsets_out = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    ops = [points, _i32c(offsets, dev), *cand, _f64c(glob, dev), out, offsets_out]
    if workspace:
        ops.append(_lib.scratch("md_cp_aug_points", (N, Ns, B), dev))
    _lib.call("md_cp_aug_points", ops)
    return out, offsets_out


def cp_aug_boxes(gt_boxes, gt_classes, gt_count, keep, glob, bv_range, cand_boxes=None, cand_classes=None, accept=None):
    """the class selection, the box side of the two flips, the rotation, the scale (velocities included) and the translation, and
    filter_gt_box_outside_range (md_cp_aug_boxes): gt_boxes [B,G,9], gt_classes [B,G] (global 1-based class, 0: a name outside
    class_names), gt_count [B], keep [B,G] u8, glob [B,7] f64, bv_range (x min, y min, x max, y max); cand_boxes [B,S,9], cand_classes
    [B,S], accept [B,S] u8 -- all three or none -> (boxes_out [B,G+S,9] f32, classes_out [B,G+S] i32: the surviving rows in front,
    zeros with class 0 behind, out_count [B] i32)."""
    g = _boxes9("cp_aug_boxes", gt_boxes)
    dev, (B, G) = g.device, g.shape[:2]
    cand = [cand_boxes, cand_classes, accept]
    if any(c is None for c in cand) != all(c is None for c in cand):
        raise ValueError("cp_aug_boxes: cand_boxes, cand_classes and accept come together")
    S = 0
    if cand_boxes is not None:
        cand = [_boxes9("cp_aug_boxes", cand_boxes), _i32c(cand_classes, dev), _u8c(accept, dev)]
        S = cand[0].shape[1]
    at = _CPBoxesAttrs((ctypes.c_float * 4)(*[float(v) for v in bv_range]))
    out = torch.empty((B, G + S, 9), dtype=torch.float32, device=dev)
    cls = torch.empty((B, G + S), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call("md_cp_aug_boxes", [g, _i32c(gt_classes, dev), _i32c(gt_count, dev), _u8c(keep, dev), *cand, _f64c(glob, dev), out, cls, count],
              extra=at)
    return out, cls, count


class CenterPointAugment:
    """The training branch of the reference's Preprocess step and the ground-truth filter of its Voxelization step
    (centerpoint/det3d_ms/datasets/pipelines/preprocess.py:46-157, 187-193) on the device, built from the reference's keys:
    global_rot_noise, global_scale_noise, global_translate_std, min_points_in_gt, plus bv_range (x min, y min, x max, y max of the
    voxel generator's range).  The database draw and the file reads of the ground-truth sampler stay with the caller, who passes the
    drawn candidates in draw order as `sampled`.

    Not built, a true / non-default value raises ValueError: flip_coor, group sampling (use_group_sampling / group_ids), the sampler's
    per-object global rotation (global_random_rotation_range_per_object other than [0, 0]), random_crop, and shuffle_points.
    shuffle_points=True is refused rather than ignored because the voxeliser is order-dependent (the first max_points points of a
    cell and the first max_voxels cells win), so a shuffle changes the result; and the merged list has a data-dependent length (the
    accepted candidates' points), so on the device a shuffle is a keyed sort of a list whose length is not known on the host -- work
    of its own, not a flag of this operator."""

    _REFUSED = ("shuffle_points", "flip_coor", "use_group_sampling", "group_ids", "random_crop", "no_augmentation", "npoints")

    def __init__(self, bv_range, global_rot_noise, global_scale_noise, global_translate_std=0, min_points_in_gt=-1, **options):
        for k, v in options.items():
            if k == "global_random_rotation_range_per_object":
                if v is not None and any(float(x) != 0.0 for x in (v if isinstance(v, (list, tuple)) else [v])):
                    raise ValueError("CenterPointAugment: the sampler's per-object global rotation is not built")
                continue
            if k not in self._REFUSED:
                raise ValueError(f"CenterPointAugment: unknown option {k!r}")
            if v not in (None, False, -1):
                raise ValueError(f"CenterPointAugment: {k} is not built")

        def pair(v):           # a scalar means [-v, v] (core/sampler/preprocess.py:666-667)
            return (-float(v), float(v)) if not isinstance(v, (list, tuple)) else (float(v[0]), float(v[1]))

        self.bv_range = tuple(float(v) for v in bv_range)
        if len(self.bv_range) != 4:
            raise ValueError("CenterPointAugment: bv_range has 4 values")
        self.global_rot_noise = pair(global_rot_noise)
        if isinstance(global_scale_noise, (list, tuple)):
            self.global_scale_noise = (float(global_scale_noise[0]), float(global_scale_noise[1]))
        else:
            raise ValueError("CenterPointAugment: global_scale_noise is (min_scale, max_scale)")
        std = global_translate_std
        std = [float(std)] * 3 if not isinstance(std, (list, tuple)) else [float(v) for v in std]
        if len(std) != 3:
            raise ValueError("CenterPointAugment: global_translate_std is a number or 3 values")
        self.global_translate_std = tuple(std)
        self.min_points_in_gt = int(min_points_in_gt)

    @classmethod
    def from_config(cls, cfg):
        """cfg.train_cfg["augment"] (the reference's keys) and the voxel generator's range"""
        r = cfg.model["voxel_generator"]["range"]
        return cls((r[0], r[1], r[3], r[4]), **dict(cfg.train_cfg["augment"]))

    def draw(self, B, generator=None, device="cuda"):
        """global [B,7] float64 on the device with the reference's distributions: two Bernoulli(0.5) (random_flip_both), the
        rotation uniform in global_rot_noise, the scale uniform in global_scale_noise, the translation normal with
        global_translate_std x, y and -- as the reference does, core/sampler/preprocess.py:825-827 -- x again for z (zeros when every
        std is 0).  From torch's generator, not numpy's stream: the reference's distributions, not its sequence."""
        if generator is not None:
            device = generator.device
        f64 = dict(dtype=torch.float64, device=device, generator=generator)
        glob = torch.empty((B, 7), dtype=torch.float64, device=device)
        glob[:, 0] = (torch.rand((B,), **f64) < 0.5).double()
        glob[:, 1] = (torch.rand((B,), **f64) < 0.5).double()
        lo, hi = self.global_rot_noise
        glob[:, 2] = lo + (hi - lo) * torch.rand((B,), **f64)
        lo, hi = self.global_scale_noise
        glob[:, 3] = lo + (hi - lo) * torch.rand((B,), **f64)
        std = self.global_translate_std
        glob[:, 4:7] = torch.randn((B, 3), **f64) * torch.tensor([std[0], std[1], std[0]], dtype=torch.float64, device=device)
        return glob

    def __call__(self, points, offsets, gt_boxes, gt_classes, gt_count, sampled=None, draws=None, generator=None):
        """points [N,5] f32, offsets [B+1] i32, gt_boxes [B,G,9] f32, gt_classes [B,G] (global 1-based class, 0: a name outside
        class_names), gt_count [B]; sampled = dict(points [Ns,5], offsets [B S + 1], boxes [B,S,9], classes [B,S], group [B,S],
        count [B]) or None; draws = global [B,7] f64 of draw() (None: drawn here with `generator`) -> dict(points, offsets, gt_boxes
        [B,G+S,9], gt_classes [B,G+S], gt_count [B], counts, keep, accept (None without `sampled`), global), nothing read back."""
        g = _boxes9("CenterPointAugment", gt_boxes)
        dev, B = g.device, g.shape[0]
        glob = self.draw(B, generator, dev) if draws is None else _f64c(draws, dev)
        counts, keep = cp_aug_count_points(points, offsets, g, gt_count, self.min_points_in_gt)
        s = dict(sampled) if sampled is not None else None
        accept = None
        if s is not None:
            missing = {"points", "offsets", "boxes", "classes", "group", "count"} - set(s)
            if missing:
                raise ValueError(f"CenterPointAugment: sampled lacks {sorted(missing)}")
            accept = cp_aug_select(g, gt_count, keep, s["boxes"], s["count"], s["group"])
            pts, offs = cp_aug_points(points, offsets, glob, s["points"], s["offsets"], s["boxes"], accept)
            boxes, classes, count = cp_aug_boxes(g, gt_classes, gt_count, keep, glob, self.bv_range, s["boxes"], s["classes"], accept)
        else:
            pts, offs = cp_aug_points(points, offsets, glob)
            boxes, classes, count = cp_aug_boxes(g, gt_classes, gt_count, keep, glob, self.bv_range)
        return dict(points=pts, offsets=offs, gt_boxes=boxes, gt_classes=classes, gt_count=count, counts=counts, keep=keep, accept=accept,
                    **{"global": glob})


# ----------------------------------------------------------------------------- CenterPoint multi-sweep input (csrc/cpsweeps.hip)
CPSWEEPS_MAX_SWEEPS, CPSWEEPS_MAX_BATCH = 32, 256     # MD_CPSWEEPS_MAX_SWEEPS, MD_CPSWEEPS_MAX_BATCH
SWEEP_REMOVE_CLOSE, SWEEP_TRANSFORM = 1, 2            # the bits of seg_flags


class _CPSweepsAttrs(ctypes.Structure):
    _fields_ = [("radius", ctypes.c_float), ("reserved0", ctypes.c_int32)]


def cp_sweeps_merge_workspace_bytes(N, B, S):
    """bytes of scratch md_cp_sweeps_merge takes (include/minddet_hip_cpsweeps.h)"""
    return _lib.workspace_bytes("md_cp_sweeps_merge", N, B, S)


def cp_sweeps_merge(points, seg_range, transforms, time_lag, seg_flags, radius=1.0, workspace=True, out=None):
    """read_sweep per segment and the concatenation of the nuScenes loader (md_cp_sweeps_merge, include/minddet_hip_cpsweeps.h):
    points [N,4 or 5] f32, one pool of rows; seg_range [B,S,2] i32 (begin, end) in output order; transforms [B,S,12] f64 (rows 0-2 of
    the 4x4); time_lag [B,S] f64; seg_flags [B,S] i32 (SWEEP_REMOVE_CLOSE | SWEEP_TRANSFORM) -> (points_out [M,5] f32 with zero rows
    behind the last kept row, offsets_out [B+1] i32, status [B] i32: bit 0 a range outside [0, N], bit 1 more than N rows in all).
    out: a [M,5] f32 tensor with M >= N to write into (None: N rows).  workspace=False leaves the scratch to the per-stream pool."""
    if points.dim() != 2 or points.shape[1] not in (4, 5):
        raise ValueError(f"cp_sweeps_merge: points are [N, 4] or [N, 5], got {tuple(points.shape)}")
    points = _f32c(points)
    dev, N = points.device, points.shape[0]
    if seg_range.dim() != 3 or seg_range.shape[2] != 2:
        raise ValueError(f"cp_sweeps_merge: seg_range is [B, S, 2], got {tuple(seg_range.shape)}")
    B, S = seg_range.shape[:2]
    for name, t, want in (("transforms", transforms, (B, S, 12)), ("time_lag", time_lag, (B, S)), ("seg_flags", seg_flags, (B, S))):
        if tuple(t.shape) != want:
            raise ValueError(f"cp_sweeps_merge: {name} is {list(want)} beside seg_range {[B, S, 2]}, got {tuple(t.shape)}")
    if out is None:
        out = torch.empty((N, 5), dtype=torch.float32, device=dev)
    elif out.dim() != 2 or out.shape[1] != 5 or out.shape[0] < N or out.dtype != torch.float32:
        raise ValueError(f"cp_sweeps_merge: out is [M, 5] f32 with M >= {N}, got {tuple(out.shape)} {out.dtype}")
    offsets_out = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    ops = [points, _i32c(seg_range, dev), _f64c(transforms, dev), _f64c(time_lag, dev), _i32c(seg_flags, dev), out, offsets_out, status]
    if workspace:
        ops.append(_lib.scratch("md_cp_sweeps_merge", (N, B, S), dev))
    _lib.call("md_cp_sweeps_merge", ops, extra=_CPSweepsAttrs(float(radius), 0))
    return out, offsets_out, status


def _sweep_order(order):
    if order not in ("key_first", "oldest_first"):
        raise ValueError(f"sweeps: order is 'key_first' (the loader) or 'oldest_first' (the deployment demo), got {order!r}")
    return order


class SweepMerger:
    """The tables of cp_sweeps_merge for the reference's two callers, built on the host (a few numbers per sweep).
    order="key_first": LoadPointCloudFromFile, nuScenes branch (centerpoint/det3d_ms/datasets/pipelines/loading.py:133-159): the key
    frame unfiltered and untransformed with time 0, then the nsweeps - 1 past sweeps in the order of the np.random.choice draw, each
    through remove_close (min_distance) and, unless its transform_matrix is None (the padding sweeps of nusc_common.py:443-450), the
    4x4.  order="oldest_first": the deployment demo (tools_ms/multi_sweep_inference_ros.py:194-270): the past sweeps oldest first,
    each transformed, the current frame last; min_distance=None filters nothing, as the demo does.
    Not built, refused with ValueError: virtual points, random_select, a dataset type other than nuScenes."""

    def __init__(self, nsweeps, min_distance=1.0, order="key_first", **options):
        for k, v in options.items():
            if k in ("virtual", "random_select"):
                if v:
                    raise ValueError(f"SweepMerger: {k} is not built")
            elif k in ("dataset", "type"):
                if v not in (None, "NuScenesDataset"):
                    raise ValueError(f"SweepMerger: the {v} branch of LoadPointCloudFromFile is not built (nuScenes only)")
            else:
                raise ValueError(f"SweepMerger: unknown option {k!r}")
        self.nsweeps, self.order = int(nsweeps), _sweep_order(order)
        if not 1 <= self.nsweeps <= CPSWEEPS_MAX_SWEEPS:
            raise ValueError(f"SweepMerger: nsweeps in [1, {CPSWEEPS_MAX_SWEEPS}], got {nsweeps}")
        self.min_distance = None if min_distance is None else float(min_distance)
        if self.min_distance is not None and not (self.min_distance >= 0 and math.isfinite(self.min_distance)):
            raise ValueError("SweepMerger: min_distance is a finite radius >= 0, or None")

    @classmethod
    def from_config(cls, cfg):
        """cfg.data["sweeps"]: nsweeps, min_distance, order (and the options that are refused)"""
        data = cfg.data if hasattr(cfg, "data") else cfg["data"]
        if "sweeps" not in data:
            raise ValueError("SweepMerger: the config has no data['sweeps'] (see configs/centerpoint/centerpoint_pp_nusc_sweeps.py)")
        return cls(**dict(data["sweeps"]))

    @property
    def radius(self):
        return 0.0 if self.min_distance is None else self.min_distance

    def tables(self, lengths, matrices, time_lags, order=None, begins=None):
        """lengths [B][nsweeps] rows per frame, frame 0 the key (current) frame, then the past sweeps as the info lists them (newest
        first); matrices [B][nsweeps] 4x4 float64 or None = no transform (frame 0's is not looked at); time_lags [B][nsweeps]
        (frame 0's is not looked at: its time is 0).  One sample may be given without the outer list.  begins [B][nsweeps]: each
        frame's first row in the pool (None: the frames lie back to back in the order given).  order, key_first only: None keeps the
        past sweeps as listed; an object with .choice (np.random, a RandomState, a Generator) draws choice(nsweeps - 1, nsweeps - 1,
        replace=False) per sample as the loader does; an array [B][nsweeps - 1] is a recorded draw.
        -> dict(seg_range [B,S,2] i32, transforms [B,S,12] f64, time_lag [B,S] f64, seg_flags [B,S] i32, order [B,S-1] i64), numpy"""
        if len(lengths) and not hasattr(lengths[0], "__len__"):
            lengths, matrices, time_lags = [lengths], [matrices], [time_lags]
            begins = None if begins is None else [begins]
            if order is not None and not hasattr(order, "choice"):
                order = [order]
        B, S = len(lengths), self.nsweeps
        if len(matrices) != B or len(time_lags) != B or any(len(x) != S for t in (lengths, matrices, time_lags) for x in t):
            raise ValueError(f"SweepMerger: lengths, matrices and time_lags are [B][{S}]")
        past = S - 1
        if order is None:
            perm = np.tile(np.arange(past, dtype=np.int64), (B, 1))
        elif hasattr(order, "choice"):
            if self.order != "key_first":
                raise ValueError("SweepMerger: the demo's order is not drawn")
            perm = np.stack([np.asarray(order.choice(past, past, replace=False), np.int64) for _ in range(B)]).reshape(B, past)
        else:
            perm = np.asarray(order, np.int64).reshape(B, past)
            if any(sorted(p.tolist()) != list(range(past)) for p in perm):
                raise ValueError("SweepMerger: order is a permutation of the past sweeps per sample")
        if self.order == "oldest_first":
            if order is not None:
                raise ValueError("SweepMerger: the demo's order is fixed")
            perm = perm[:, ::-1]
        seg = np.zeros((B, S, 2), np.int32)
        tf = np.tile(np.eye(4)[:3].reshape(12), (B, S, 1))
        lag = np.zeros((B, S), np.float64)
        flags = np.zeros((B, S), np.int32)
        filt = SWEEP_REMOVE_CLOSE if self.min_distance is not None else 0
        at = 0
        for b in range(B):
            start = []
            for i in range(S):
                start.append(at if begins is None else int(begins[b][i]))
                at += int(lengths[b][i])
            frames = [1 + int(i) for i in perm[b]]
            frames = [0] + frames if self.order == "key_first" else frames + [0]
            for s, i in enumerate(frames):
                seg[b, s] = (start[i], start[i] + int(lengths[b][i]))
                if i == 0:
                    continue
                lag[b, s] = float(time_lags[b][i])
                flags[b, s] = filt
                if matrices[b][i] is not None:
                    m = np.asarray(matrices[b][i], np.float64)
                    if m.shape != (4, 4):
                        raise ValueError(f"SweepMerger: a transform is a 4x4, got {m.shape}")
                    tf[b, s] = m[:3].reshape(12)
                    flags[b, s] |= SWEEP_TRANSFORM
        return dict(seg_range=seg, transforms=tf, time_lag=lag, seg_flags=flags, order=perm.copy())

    def __call__(self, points, lengths, matrices, time_lags, order=None, begins=None, out=None):
        """tables(), four small host-to-device copies, then cp_sweeps_merge on the pool `points` -> (points, offsets, status)"""
        t = self.tables(lengths, matrices, time_lags, order=order, begins=begins)
        dev = points.device
        return cp_sweeps_merge(points, *[torch.from_numpy(t[k]).to(dev) for k in ("seg_range", "transforms", "time_lag", "seg_flags")],
                               radius=self.radius, out=out)


class SweepRing:
    """The streaming form of the deployment demo (tools_ms/multi_sweep_inference_ros.py:194-270): a ring of the last nsweeps frames in
    ONE [nsweeps slot_rows, Fin] device buffer.  push() copies the new frame device-to-device into the slot of the frame it evicts and
    merges the frames held into the newest frame with one cp_sweeps_merge call whose ranges point into the ring: a past frame is never
    copied again.  The poses arrive on the host (16 numbers per frame): inv(G_newest) @ G_i is composed there in numpy float64.
    order="oldest_first": the demo's, the current frame last; "key_first": the current frame, then the past frames newest first.
    min_distance=None filters nothing (the demo); a radius applies remove_close to the past frames."""

    def __init__(self, nsweeps, slot_rows, order="oldest_first", min_distance=None, device="cuda"):
        self.merger = SweepMerger(nsweeps, min_distance=min_distance, order=order)
        self.nsweeps, self.slot_rows, self.device = self.merger.nsweeps, int(slot_rows), torch.device(device)
        if self.slot_rows < 1 or self.nsweeps * self.slot_rows >= 1 << 30:
            raise ValueError("SweepRing: slot_rows >= 1 and nsweeps slot_rows < 2^30")
        self.buffer = None
        self.frames = []        # (slot, rows, global_from_lidar 4x4 float64, stamp), oldest first
        self.pushed = 0

    def matrices(self):
        """[len(frames)] 4x4 float64, oldest first: inv(G_newest) @ G_i (the newest frame's is the identity up to rounding)"""
        inv = np.linalg.inv(self.frames[-1][2])
        return [inv @ g for _, _, g, _ in self.frames]

    def tables(self):
        """the four tables of the frames held (B = 1, S = nsweeps; the segments of frames not yet pushed are empty), numpy"""
        held = self.frames[::-1]                                  # newest first: frame 0 is the current one, as SweepMerger takes them
        mats = self.matrices()[::-1]
        pad = self.nsweeps - len(held)
        lengths = [n for _, n, _, _ in held] + [0] * pad
        begins = [slot * self.slot_rows for slot, _, _, _ in held] + [0] * pad
        newest = held[0][3]
        lags = [float(newest) - float(st) for _, _, _, st in held] + [0.0] * pad
        return self.merger.tables(lengths, [None] + mats[1:] + [None] * pad, lags, begins=begins)

    def admit(self, rows, global_from_lidar, stamp):
        """the host side of push(): a frame of `rows` rows takes the slot of the frame it evicts -> the slot"""
        n = int(rows)
        if n > self.slot_rows:
            raise ValueError(f"SweepRing: a frame of {n} rows does not fit a slot of {self.slot_rows}")
        g = np.asarray(global_from_lidar, np.float64)
        if g.shape != (4, 4):
            raise ValueError(f"SweepRing: global_from_lidar is a 4x4, got {g.shape}")
        slot = self.pushed % self.nsweeps
        if len(self.frames) == self.nsweeps:
            self.frames.pop(0)                                    # the oldest frame: its slot is the one overwritten
        self.frames.append((slot, n, g.copy(), float(stamp)))
        self.pushed += 1
        return slot

    def push(self, points, global_from_lidar, stamp):
        """points [n,4 or 5] f32 on the device, n <= slot_rows; global_from_lidar 4x4 float64 (host); stamp in seconds
        -> (points [nsweeps slot_rows,5], offsets [2], status [1]) of the merged cloud in this frame, time = stamp - stamp_i"""
        if points.dim() != 2 or points.shape[1] not in (4, 5):
            raise ValueError(f"SweepRing: points are [n, 4] or [n, 5], got {tuple(points.shape)}")
        if self.buffer is not None and points.shape[1] != self.buffer.shape[1]:
            raise ValueError(f"SweepRing: the ring holds {self.buffer.shape[1]}-wide points, got {points.shape[1]}")
        n = points.shape[0]
        slot = self.admit(n, global_from_lidar, stamp)
        if self.buffer is None:
            self.buffer = torch.zeros((self.nsweeps * self.slot_rows, points.shape[1]), dtype=torch.float32, device=self.device)
        self.buffer[slot * self.slot_rows:slot * self.slot_rows + n].copy_(points)
        t = self.tables()
        return cp_sweeps_merge(self.buffer, *[torch.from_numpy(t[k]).to(self.device) for k in ("seg_range", "transforms", "time_lag", "seg_flags")],
                               radius=self.merger.radius)


# ----------------------------------------------------------------------------- training operators: outputs, head losses
def _out_dict(who, want, out, dev):
    """want: {key: (shape, dtype)} -> `out` checked against it, or a new dict of empty tensors on dev"""
    if out is None:
        out = {k: torch.empty(shp, dtype=dt, device=dev) for k, (shp, dt) in want.items()}
    for k, (shp, dt) in want.items():
        if tuple(out[k].shape) != shp or out[k].dtype != dt:
            raise ValueError(f"{who}: out[{k!r}] has to be {dt} of shape {shp}")
    return out


def _bf16_head(who, head, layout):
    if head.dtype != torch.bfloat16 or head.dim() != 4:
        raise ValueError(f"{who}: head has to be {layout} bfloat16")
    return head.contiguous()


def _head_loss(who, sym, head, operands, want, ws_dims, at, grad, out):
    """One call of a loss over a merged head tensor (the head _bf16_head returned): `sym`(head, *operands, parts, num_pos, total,
    workspace) or, with grad, `sym`_grad with grad (head's shape, f32) in front of the workspace.  want: (shape, dtype) of parts and
    num_pos; ws_dims: the extents `sym`_workspace_bytes takes -> the dict of total, parts, num_pos [, grad]."""
    want = dict(total=((1,), torch.float32), **want)
    if grad:
        want["grad"] = (tuple(head.shape), torch.float32)
    out = _out_dict(who, want, out, head.device)
    ws = _lib.scratch(sym, ws_dims, head.device)
    outs = [out["parts"], out["num_pos"], out["total"]] + ([out["grad"]] if grad else [])
    _lib.call(sym + "_grad" if grad else sym, [head, *operands, *outs, ws], extra=at)
    return out


class _HeadLossFn(torch.autograd.Function):
    """call(head) -> the dict of a *_loss with grad=True; the differentiable form of all three"""

    @staticmethod
    def forward(ctx, head, call):
        out = call(head.detach())
        ctx.save_for_backward(out["grad"])
        ctx.head_dtype = head.dtype
        ctx.mark_non_differentiable(out["parts"], out["num_pos"])
        return out["total"], out["parts"], out["num_pos"]

    @staticmethod
    def backward(ctx, g_total, g_parts, g_num_pos):
        (grad,) = ctx.saved_tensors
        return (g_total.to(torch.float32) * grad).to(ctx.head_dtype), None


# ----------------------------------------------------------------------------- CenterPoint training targets (csrc/cptargets.hip)
class _CPTargetsAttrs(ctypes.Structure):
    _fields_ = [("num_tasks", ctypes.c_int32), ("num_classes", ctypes.c_int32 * 8), ("voxel_size", ctypes.c_float * 2),
                ("pc_range", ctypes.c_float * 2), ("out_size_factor", ctypes.c_int32), ("gaussian_overlap", ctypes.c_float),
                ("min_radius", ctypes.c_int32)]


def _task_num_classes(tasks):
    """per task num_class, from the config's task dicts (or plain integers)"""
    return [int(t if isinstance(t, int) else t["num_class"]) for t in tasks]


def cp_assign_targets(gt_boxes, gt_classes, *, tasks, voxel_size, pc_range, out_size_factor, gaussian_overlap, min_radius, max_objs,
                      feature_map_size, out=None):
    """AssignLabel.__call__ (preprocess.py:297-521) for a batch on the device (md_cp_assign_targets, include/minddet_hip_cptargets.h):
    gt_boxes [B,G,9] f32 (x, y, z, w, l, h, vx, vy, rot), gt_classes [B,G] (global 1-based class; 0 or an id past the last class: a
    padding row), G <= max_objs -> dict with the reference's keys: hm [B,T,C,H,W] f32, anno_box [B,T,M,10] f32, ind [B,T,M] i32,
    mask [B,T,M] u8, cat [B,T,M] i32, gt_boxes_and_cls [B,M,10] f32.  feature_map_size = (W, H) as in the reference; every element
    of every output is written by the op, so `out` (a dict of such tensors from an earlier call) can be reused without clearing."""
    ncs = _task_num_classes(tasks)
    if not 1 <= len(ncs) <= CP_MAX_TASKS:
        raise ValueError(f"cp_assign_targets: 1 .. {CP_MAX_TASKS} tasks, got {len(ncs)}")
    at = _CPTargetsAttrs()
    at.num_tasks = len(ncs)
    for t, nc in enumerate(ncs):
        at.num_classes[t] = nc
    for i in range(2):
        at.voxel_size[i], at.pc_range[i] = float(voxel_size[i]), float(pc_range[i])
    at.out_size_factor, at.gaussian_overlap, at.min_radius = int(out_size_factor), float(gaussian_overlap), int(min_radius)
    g = _f32c(gt_boxes)
    dev = g.device
    cls = gt_classes.to(device=dev, dtype=torch.int32).contiguous()
    B, G = g.shape[0], g.shape[1]
    T, C, M = len(ncs), max(ncs), int(max_objs)
    W, H = int(feature_map_size[0]), int(feature_map_size[1])
    want = dict(hm=((B, T, C, H, W), torch.float32), anno_box=((B, T, M, 10), torch.float32), ind=((B, T, M), torch.int32),
                mask=((B, T, M), torch.uint8), cat=((B, T, M), torch.int32), gt_boxes_and_cls=((B, M, 10), torch.float32))
    out = _out_dict("cp_assign_targets", want, out, dev)
    ws = _lib.scratch("md_cp_assign_targets", (B, T, G), dev)
    _lib.call("md_cp_assign_targets", [g, cls, out["hm"], out["anno_box"], out["ind"], out["mask"], out["cat"], out["gt_boxes_and_cls"], ws],
              extra=at)
    return out


class CenterPointTargets:
    """The AssignLabel step of a config: train_cfg["assigner"] (target_assigner.tasks, out_size_factor, gaussian_overlap, max_objs,
    min_radius -- the reference's key names) plus the voxel generator's range and voxel size.  __call__(gt_boxes [B,G,9],
    gt_classes [B,G]) -> the dict of cp_assign_targets."""

    def __init__(self, assigner, voxel_generator):
        self.tasks = [dict(t) for t in assigner["target_assigner"]["tasks"]]
        self.out_size_factor = int(assigner["out_size_factor"])
        self.gaussian_overlap = float(assigner["gaussian_overlap"])
        self.max_objs, self.min_radius = int(assigner["max_objs"]), int(assigner["min_radius"])
        rg, vs = voxel_generator["range"], voxel_generator["voxel_size"]
        self.pc_range, self.voxel_size = (float(rg[0]), float(rg[1])), (float(vs[0]), float(vs[1]))
        # grid_size = round((range[3:] - range[:3]) / voxel_size), feature_map_size = grid_size[:2] // out_size_factor (preprocess.py:313-318)
        grid = [int(np.round((np.float32(rg[3 + i]) - np.float32(rg[i])) / np.float32(vs[i]))) for i in range(2)]
        self.feature_map_size = (grid[0] // self.out_size_factor, grid[1] // self.out_size_factor)

    @classmethod
    def from_config(cls, cfg):
        return cls(cfg.train_cfg["assigner"], cfg.model["voxel_generator"])

    def __call__(self, gt_boxes, gt_classes):
        return cp_assign_targets(gt_boxes, gt_classes, tasks=self.tasks, voxel_size=self.voxel_size, pc_range=self.pc_range,
                                 out_size_factor=self.out_size_factor, gaussian_overlap=self.gaussian_overlap, min_radius=self.min_radius,
                                 max_objs=self.max_objs, feature_map_size=self.feature_map_size)


# ----------------------------------------------------------------------------- CenterPoint training loss (csrc/cploss.hip)
class _CPLossAttrs(ctypes.Structure):
    _fields_ = [("num_tasks", ctypes.c_int32), ("task", _CPTaskAttrs * CP_MAX_TASKS), ("weight", ctypes.c_float),
                ("code_weights", ctypes.c_float * 10)]


def cp_loss_attrs(task_offsets, num_classes, weight, code_weights):
    """md_cp_loss_attrs of a CenterHead (per task {head: first channel}, per task num_class), the loc-loss weight and the code weights
    in the order of anno_box (reg 2, height 1, dim 3, vel 2, rot 2; 8 values for heads without vel: the last two are then unused)"""
    if not 1 <= len(task_offsets) <= CP_MAX_TASKS or len(task_offsets) != len(num_classes):
        raise ValueError(f"cp_loss_attrs: 1 .. {CP_MAX_TASKS} tasks, one num_class each; got {len(task_offsets)} / {len(num_classes)}")
    cw = [float(v) for v in code_weights]
    if len(cw) not in (8, 10) or (len(cw) == 8 and any("vel" in off for off in task_offsets)):
        raise ValueError(f"cp_loss_attrs: 10 code weights (8 for heads without vel), got {len(cw)}")
    at = _CPLossAttrs()
    at.num_tasks = len(task_offsets)
    for t, (off, nc) in enumerate(zip(task_offsets, num_classes)):
        a = at.task[t]
        a.off_reg, a.off_height, a.off_dim, a.off_rot = int(off["reg"]), int(off["height"]), int(off["dim"]), int(off["rot"])
        a.off_vel, a.off_hm, a.num_classes, a.class_base = int(off.get("vel", -1)), int(off["hm"]), int(nc), 0
    at.weight = float(weight)
    for j, v in enumerate(cw):
        at.code_weights[j] = v
    return at


def cp_loss_workspace_bytes(B, T, H, W):
    return _lib.workspace_bytes("md_cp_loss", B, T, H, W)


def cp_loss(head, targets, at, grad=False, out=None):
    """CenterHead.loss (center_head.py:208-271, FastFocalLoss + RegLoss per task) on the device (md_cp_loss / md_cp_loss_grad,
    include/minddet_hip_cploss.h): head [B,H,W,Cp] bf16 raw logits in the layout of CenterHead.task_offsets(), targets = the dict of
    cp_assign_targets (hm, anno_box, ind, mask, cat) -> dict with total [1] f32, parts [T,12] f32 (per task hm_loss, loc_loss,
    box_loss[10]), num_pos [T] f32 and, with grad=True, grad [B,H,W,Cp] f32 = d total / d head.  Every element of every output is
    written, so `out` (such a dict from an earlier call) can be reused without clearing.  A slot whose ind or cat is out of range is
    skipped as if masked."""
    head = _bf16_head("cp_loss", head, "[B,H,W,Cp]")
    B, H, W, _ = head.shape
    T = int(at.num_tasks)
    want = dict(parts=((T, 12), torch.float32), num_pos=((T,), torch.float32))
    return _head_loss("cp_loss", "md_cp_loss", head, [targets[k] for k in ("hm", "anno_box", "ind", "mask", "cat")], want,
                      (B, T, H, W), at, grad, out)


class CenterPointLoss:
    """The loss of a CenterHead: its channel layout plus the loc-loss weight and the code weights (the reference's CenterHead
    arguments `weight` and `code_weights`).  __call__(head, targets, grad=False) -> the dict of cp_loss."""

    def __init__(self, task_offsets, num_classes, weight=0.25, code_weights=(1.0,) * 10):
        self.weight, self.code_weights = float(weight), [float(v) for v in code_weights]
        self.num_classes = [int(n) for n in num_classes]
        self.at = cp_loss_attrs(task_offsets, self.num_classes, self.weight, self.code_weights)

    @classmethod
    def from_head(cls, center_head, weight=None, code_weights=None):
        """weight / code_weights None: the values the head was built with"""
        weight = center_head.weight if weight is None else weight
        code_weights = center_head.code_weights if code_weights is None else code_weights
        return cls(center_head.task_offsets(), center_head.num_classes, weight, code_weights)

    @classmethod
    def from_config(cls, cfg, center_head):
        loss = cfg.train_cfg["loss"]
        return cls.from_head(center_head, loss["weight"], loss["code_weights"])

    def __call__(self, head, targets, grad=False, out=None):
        return cp_loss(head, targets, self.at, grad=grad, out=out)


def center_point_loss(head, targets, loss):
    """differentiable form: -> (total [1] f32, parts [T,12], num_pos [T]); the forward runs md_cp_loss_grad once, the backward returns
    grad_output x (d total / d head) in the head's dtype.  parts and num_pos carry no gradient."""
    return _HeadLossFn.apply(head, lambda h: cp_loss(h, targets, loss.at, grad=True))


# ----------------------------------------------------------------------------- KITTI PointPillars training loss (csrc/pploss.hip)
class _PPLossAttrs(ctypes.Structure):
    _fields_ = [("head", _PPHeadAttrs), ("alpha", ctypes.c_float), ("gamma", ctypes.c_float), ("sigma", ctypes.c_float),
                ("code_weights", ctypes.c_float * 7), ("cls_weight", ctypes.c_float), ("loc_weight", ctypes.c_float),
                ("dir_weight", ctypes.c_float), ("pos_cls_weight", ctypes.c_float), ("neg_cls_weight", ctypes.c_float)]


def pp_loss_attrs(head_offsets, num_anchors, num_classes, alpha=0.25, gamma=2.0, sigma=3.0, code_weights=(1.0,) * 7, cls_weight=1.0,
                  loc_weight=2.0, dir_weight=0.2, pos_cls_weight=1.0, neg_cls_weight=1.0):
    """md_pp_loss_attrs: head_offsets = PPAnchorHead.head_offsets() ({cls, box, dir_cls}: first channels; dir_cls None = no direction
    loss), alpha None = no alpha factor; the other names are the reference configuration's (classification_loss.alpha / gamma,
    localization_loss.sigma / code_weight, classification_weight, localization_weight, direction_loss_weight, pos_class_weight,
    neg_class_weight).  The defaults are the values of both KITTI configurations."""
    cw = [float(v) for v in code_weights]
    if len(cw) != 7:
        raise ValueError(f"pp_loss_attrs: 7 code weights, got {len(cw)}")
    off_dir = head_offsets.get("dir_cls")
    at = _PPLossAttrs()
    at.head = _PPHeadAttrs(int(head_offsets["cls"]), int(head_offsets["box"]), -1 if off_dir is None else int(off_dir), int(num_anchors),
                           int(num_classes), 0, 1)
    if alpha is not None and float(alpha) < 0:
        raise ValueError("pp_loss_attrs: alpha is None or >= 0")
    at.alpha, at.gamma, at.sigma = -1.0 if alpha is None else float(alpha), float(gamma), float(sigma)
    for j, v in enumerate(cw):
        at.code_weights[j] = v
    at.cls_weight, at.loc_weight, at.dir_weight = float(cls_weight), float(loc_weight), float(dir_weight)
    at.pos_cls_weight, at.neg_cls_weight = float(pos_cls_weight), float(neg_cls_weight)
    return at


def pp_loss_workspace_bytes(B, H, W, num_anchors):
    return _lib.workspace_bytes("md_pp_loss", B, H, W, num_anchors)


def pp_loss(head, labels, reg_targets, anchors, at, grad=False, out=None):
    """PointPillarsWithLossCell.construct behind the network (pointpillars/src/pointpillars.py:817-872 with src/core/losses.py:40-191)
    on the device (md_pp_loss / md_pp_loss_grad, include/minddet_hip_pploss.h): head [B,H,W,C] bf16 raw outputs in the layout of
    PPAnchorHead.head_offsets(), labels [B,N] i32 and reg_targets [B,N,7] f32 (assign_targets_batch), anchors [N,7] f32 -> dict with
    total [1] f32, parts [5] f32 (loc, cls, dir as they enter the total, cls_pos, cls_neg), num_pos [B] f32 and, with grad=True, grad
    [B,H,W,C] f32 = d total / d head.  Every element of every output is written, so `out` (such a dict from an earlier call) can be
    reused without clearing."""
    head = _bf16_head("pp_loss", head, "[B,H,W,C]")
    B, H, W, _ = head.shape
    A = int(at.head.num_anchors)
    n = H * W * A
    if tuple(labels.shape) != (B, n) or labels.dtype != torch.int32 or tuple(reg_targets.shape) != (B, n, 7):
        raise ValueError(f"pp_loss: labels has to be int32 [{B}, {n}] and reg_targets [{B}, {n}, 7], got {tuple(labels.shape)} "
                         f"{labels.dtype} / {tuple(reg_targets.shape)}")
    want = dict(parts=((5,), torch.float32), num_pos=((B,), torch.float32))
    return _head_loss("pp_loss", "md_pp_loss", head, [labels.contiguous(), _f32c(reg_targets), _f32c(anchors).reshape(-1, 7)], want,
                      (B, H, W, A), at, grad, out)


class PointPillarsLoss:
    """The loss of a KITTI PointPillars model: the head's channel layout plus the reference configuration's loss settings (the keys of
    its `loss` block, direction_loss_weight, pos_class_weight, neg_class_weight).  __call__(head, labels, reg_targets, anchors,
    grad=False) -> the dict of pp_loss."""

    def __init__(self, head_offsets, num_anchors, num_classes, loss=None, direction_loss_weight=0.2, pos_class_weight=1.0,
                 neg_class_weight=1.0):
        loss = dict(loss or {})
        cls_cfg, loc_cfg = dict(loss.get("classification_loss", {})), dict(loss.get("localization_loss", {}))
        self.head_offsets, self.num_anchors, self.num_classes = dict(head_offsets), int(num_anchors), int(num_classes)
        self.alpha, self.gamma = cls_cfg.get("alpha", 0.25), float(cls_cfg.get("gamma", 2.0))
        self.sigma = float(loc_cfg.get("sigma", 3.0))
        self.code_weights = [float(v) for v in (loc_cfg.get("code_weight") or [1.0] * 7)]
        self.cls_weight, self.loc_weight = float(loss.get("classification_weight", 1.0)), float(loss.get("localization_weight", 2.0))
        self.dir_weight = float(direction_loss_weight)
        self.pos_cls_weight, self.neg_cls_weight = float(pos_class_weight), float(neg_class_weight)
        self.at = pp_loss_attrs(self.head_offsets, self.num_anchors, self.num_classes, self.alpha, self.gamma, self.sigma, self.code_weights,
                                self.cls_weight, self.loc_weight, self.dir_weight, self.pos_cls_weight, self.neg_cls_weight)

    @classmethod
    def from_net(cls, net, train_cfg=None):
        """net: a graphs.PointPillarsNet (or the from-points model that wraps one); train_cfg: the config's train_cfg (its "loss" block
        and the three weights beside it); None = the values of the KITTI configurations"""
        net = getattr(net, "inner", net)
        t = dict(train_cfg or {})
        return cls(net.head_offsets(), net.num_anchors, net.num_class, t.get("loss"), t.get("direction_loss_weight", 0.2),
                   t.get("pos_class_weight", 1.0), t.get("neg_class_weight", 1.0))

    @classmethod
    def from_config(cls, cfg, net):
        return cls.from_net(net, cfg.train_cfg)

    def __call__(self, head, labels, reg_targets, anchors, grad=False, out=None):
        return pp_loss(head, labels, reg_targets, anchors, self.at, grad=grad, out=out)


def point_pillars_loss(head, labels, reg_targets, anchors, loss):
    """differentiable form: -> (total [1] f32, parts [5], num_pos [B]); the forward runs md_pp_loss_grad once, the backward returns
    grad_output x (d total / d head) in the head's dtype.  parts and num_pos carry no gradient."""
    return _HeadLossFn.apply(head, lambda h: pp_loss(h, labels, reg_targets, anchors, loss.at, grad=True))


def assign_targets_batch(anchors, gt_boxes, gt_classes, matched_thr, unmatched_thr, anchors_mask=None):
    """assign_targets for a batch: gt_boxes / gt_classes are per-sample lists ([G_b,7] / [G_b] or None), anchors_mask [B,N] or None
    -> (labels [B,N] i32, bbox_targets [B,N,7] f32, bbox_outside_weights [B,N] f32, gt_ids [B,N] i32), the inputs of pp_loss.  One
    md_assign_targets call per sample (no new kernel), nothing read back."""
    B = len(gt_boxes)
    if B < 1 or (gt_classes is not None and len(gt_classes) != B) or (anchors_mask is not None and len(anchors_mask) != B):
        raise ValueError("assign_targets_batch: one gt_boxes / gt_classes / anchors_mask entry per sample, at least one sample")
    rows = [assign_targets(anchors, gt_boxes[b], None if gt_classes is None else gt_classes[b], matched_thr, unmatched_thr,
                           None if anchors_mask is None else anchors_mask[b]) for b in range(B)]
    return tuple(torch.stack([r[i] for r in rows]) for i in range(4))


# ----------------------------------------------------------------------------- CenterNet training targets (csrc/cntargets.hip)
CN_MAX_OBJS = 1024            # MD_CN_MAX_OBJS


class _CNTargetsAttrs(ctypes.Structure):
    _fields_ = [("min_overlap", ctypes.c_float)]


def cn_assign_targets(boxes, classes, *, num_classes, feature_map_size, max_objs, min_overlap=0.7, out=None):
    """The target part of COCOHP.preprocess_fn (centernet/src/dataset.py:343-359) for a batch on the device (md_cn_assign_targets,
    include/minddet_hip_cn.h): boxes [B,G,4] f32 (x0, y0, x1, y1 in output-map coordinates, after the flip and the affine transform,
    before the clip), classes [B,G] (1-based category_id; < 1 or > num_classes: a padding row), G <= max_objs -> dict with the
    reference's keys: hm [B,C,H,W] f32, ind [B,M] i32, reg_mask [B,M] u8, wh [B,M,2] f32, reg [B,M,2] f32.  feature_map_size = (W, H);
    every element of every output is written by the op, so `out` (such a dict from an earlier call) can be reused without clearing."""
    at = _CNTargetsAttrs(float(min_overlap))
    g = _f32c(boxes)
    dev = g.device
    cls = classes.to(device=dev, dtype=torch.int32).contiguous()
    B, G = g.shape[0], g.shape[1]
    C, M = int(num_classes), int(max_objs)
    W, H = int(feature_map_size[0]), int(feature_map_size[1])
    want = dict(hm=((B, C, H, W), torch.float32), ind=((B, M), torch.int32), reg_mask=((B, M), torch.uint8), wh=((B, M, 2), torch.float32),
                reg=((B, M, 2), torch.float32))
    out = _out_dict("cn_assign_targets", want, out, dev)
    ws = _lib.scratch("md_cn_assign_targets", (B, M), dev)
    _lib.call("md_cn_assign_targets", [g, cls, out["hm"], out["ind"], out["reg_mask"], out["wh"], out["reg"], ws], extra=at)
    return out


class CenterNetTargets:
    """The target step of a CenterNet config: num_classes, the output map (input_res // down_ratio), max_objs and min_overlap.
    __call__(bboxes [B,G,4] original-image boxes, category_id [B,G], trans [B,2,3] float64 `trans_output` matrices or None,
    flip_width [B] (the image width of a flipped sample, 0 or less: not flipped) or None) -> the dict of cn_assign_targets.  The flip
    (`width - x[2,0] - 1` in fp32, dataset.py:340) and affine_transform (image.py:59-63: ((t00 x + t01 y) + t02) in float64, rounded to
    fp32) are elementwise torch ops on the device; rows past max_objs are dropped (dataset.py:274).  trans None: the boxes are
    output-map boxes already."""

    def __init__(self, num_classes=80, feature_map_size=(128, 128), max_objs=128, min_overlap=0.7):
        self.num_classes, self.max_objs, self.min_overlap = int(num_classes), int(max_objs), float(min_overlap)
        self.feature_map_size = (int(feature_map_size[0]), int(feature_map_size[1]))

    @classmethod
    def from_config(cls, cfg):
        a = cfg.train_cfg["assigner"]
        h, w = (int(v) for v in a["input_res"])
        d = int(a["down_ratio"])
        return cls(cfg.model["num_classes"], (w // d, h // d), a["max_objs"], a.get("min_overlap", 0.7))

    def __call__(self, bboxes, category_id, trans=None, flip_width=None, out=None):
        b = _f32c(bboxes)[:, :self.max_objs]
        cls = category_id[:, :self.max_objs]
        dev = b.device
        if flip_width is not None:
            fw = torch.as_tensor(flip_width, device=dev).to(torch.float32).reshape(-1, 1)
            flipped = fw > 0
            x0 = torch.where(flipped, fw - b[..., 2] - 1.0, b[..., 0])
            x1 = torch.where(flipped, fw - b[..., 0] - 1.0, b[..., 2])
            b = torch.stack((x0, b[..., 1], x1, b[..., 3]), -1)
        if trans is not None:
            t = torch.as_tensor(trans, device=dev).to(torch.float64).reshape(-1, 1, 2, 3)
            pts = b.to(torch.float64).reshape(b.shape[0], b.shape[1], 2, 1, 2)       # [B,G,corner,1,(x, y)]
            tt = t.unsqueeze(2)                                                       # [B,1,1,2,3]
            b = ((tt[..., 0] * pts[..., 0] + tt[..., 1] * pts[..., 1]) + tt[..., 2]).to(torch.float32).reshape(b.shape[0], b.shape[1], 4)
        return cn_assign_targets(b, cls, num_classes=self.num_classes, feature_map_size=self.feature_map_size, max_objs=self.max_objs,
                                 min_overlap=self.min_overlap, out=out)


# ----------------------------------------------------------------------------- CenterNet training loss (csrc/cnloss.hip)
class _CNLossAttrs(ctypes.Structure):
    _fields_ = [("num_classes", ctypes.c_int32), ("off_hm", ctypes.c_int32), ("off_wh", ctypes.c_int32), ("off_reg", ctypes.c_int32),
                ("hm_weight", ctypes.c_float), ("wh_weight", ctypes.c_float), ("off_weight", ctypes.c_float)]


def cn_loss_attrs(num_classes, off_hm=0, off_wh=None, off_reg=None, hm_weight=1.0, wh_weight=0.1, off_weight=1.0, reg_offset=True):
    """md_cn_loss_attrs: the heads' first channels in the layout of graphs.CenterNet.features (hm at 0, wh behind it, reg behind wh;
    reg_offset False: no offset head) and the reference's hm_weight / wh_weight / off_weight (default_config.yaml: 1, 0.1, 1)"""
    nc = int(num_classes)
    off_wh = int(off_hm) + nc if off_wh is None else int(off_wh)
    off_reg = (off_wh + 2 if off_reg is None else int(off_reg)) if reg_offset else -1
    return _CNLossAttrs(nc, int(off_hm), off_wh, off_reg, float(hm_weight), float(wh_weight), float(off_weight))


def cn_loss_workspace_bytes(B, C, H, W):
    return _lib.workspace_bytes("md_cn_loss", B, C, H, W)


def cn_loss(head, targets, at, grad=False, out=None):
    """CenterNetLossCell.construct behind the network (centernet_det.py:177-237, FocalLoss + two RegLoss) on the device (md_cn_loss /
    md_cn_loss_grad, include/minddet_hip_cn.h): head [B,H,W,Cp] bf16 raw logits in the layout of graphs.CenterNet.features, targets =
    the dict of cn_assign_targets (hm, ind, reg_mask, wh, reg) -> dict with total [1] f32, parts [3] f32 (hm_loss, wh_loss, off_loss),
    num_pos [1] f32 and, with grad=True, grad [B,H,W,Cp] f32 = d total / d head.  Every element of every output is written, so `out`
    (such a dict from an earlier call) can be reused without clearing.  A slot whose ind is out of range is skipped as if masked."""
    head = _bf16_head("cn_loss", head, "[B,H,W,Cp]")
    B, H, W, _ = head.shape
    want = dict(parts=((3,), torch.float32), num_pos=((1,), torch.float32))
    return _head_loss("cn_loss", "md_cn_loss", head, [targets[k] for k in ("hm", "ind", "reg_mask", "wh", "reg")], want,
                      (B, int(at.num_classes), H, W), at, grad, out)


class CenterNetLoss:
    """The loss of a CenterNet head: its channel layout plus the reference's net_config loss settings.  Only the configuration the
    reference trains is built: FocalLoss on the heat map and L1 RegLoss on wh / reg of one stack; mse_loss, dense_wh, cat_spec_wh,
    another reg_loss or num_stacks != 1 raise ValueError.  __call__(head, targets, grad=False) -> the dict of cn_loss."""

    def __init__(self, num_classes=80, off_hm=0, hm_weight=1.0, wh_weight=0.1, off_weight=1.0, reg_offset=True, reg_loss="l1",
                 mse_loss=False, dense_wh=False, cat_spec_wh=False, num_stacks=1):
        given = dict(mse_loss=mse_loss, dense_wh=dense_wh, cat_spec_wh=cat_spec_wh, reg_loss=reg_loss, num_stacks=num_stacks)
        built = dict(mse_loss=False, dense_wh=False, cat_spec_wh=False, reg_loss="l1", num_stacks=1)
        for name, v in given.items():
            if v != built[name]:
                raise ValueError(f"CenterNetLoss: {name}={v!r} is not built (only {name}={built[name]!r} is)")
        self.num_classes, self.reg_offset = int(num_classes), bool(reg_offset)
        self.hm_weight, self.wh_weight, self.off_weight = float(hm_weight), float(wh_weight), float(off_weight)
        self.at = cn_loss_attrs(self.num_classes, off_hm, None, None, self.hm_weight, self.wh_weight, self.off_weight, self.reg_offset)

    @classmethod
    def from_config(cls, cfg, num_classes=None):
        loss = dict(cfg.train_cfg.get("loss", {}))
        return cls(cfg.model["num_classes"] if num_classes is None else num_classes, **loss)

    @classmethod
    def from_model(cls, net, train_cfg=None):
        """net: a graphs.CenterNet; train_cfg: a config's train_cfg (its "loss" block), None = the reference's default values"""
        return cls(net.num_classes, **dict((train_cfg or {}).get("loss", {})))

    def __call__(self, head, targets, grad=False, out=None):
        return cn_loss(head, targets, self.at, grad=grad, out=out)


def center_net_loss(head, targets, loss):
    """differentiable form: -> (total [1] f32, parts [3], num_pos [1]); the forward runs md_cn_loss_grad once, the backward returns
    grad_output x (d total / d head) in the head's dtype.  parts and num_pos carry no gradient."""
    return _HeadLossFn.apply(head, lambda h: cn_loss(h, targets, loss.at, grad=True))


# ----------------------------------------------------------------------------- CenterNet training input (csrc/cnaug.hip)
CNAUG_MAX_BATCH = 65535       # MD_CNAUG_MAX_BATCH
CN_COLOUR_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))   # 0 brightness_, 1 contrast_, 2 saturation_


class _CNAugTransformAttrs(ctypes.Structure):
    _fields_ = [("rand_crop", ctypes.c_int32), ("scale", ctypes.c_double), ("shift", ctypes.c_double), ("flip_prop", ctypes.c_double),
                ("in_h", ctypes.c_int32), ("in_w", ctypes.c_int32), ("down_ratio", ctypes.c_int32)]


class _CNAugImageAttrs(ctypes.Structure):
    _fields_ = [("out_h", ctypes.c_int32), ("out_w", ctypes.c_int32), ("pad_lo", ctypes.c_int32), ("pad_hi", ctypes.c_int32)]


def _sizes2(who, sizes, dev):
    s = _i32c(sizes, dev)
    if s.dim() != 2 or s.shape[1] != 2:
        raise ValueError(f"{who}: sizes are [B, 2] (h, w), got {tuple(s.shape)}")
    return s


def cn_aug_transform(sizes, draws, *, rand_crop, scale, shift, flip_prop, input_hw, down_ratio):
    """The random block of COCOHP.preprocess_fn and its two matrices (md_cn_aug_transform, include/minddet_hip_cnaug.h): sizes [B,2]
    (h, w) of the source images, draws [B,4] f64 (the values the reference drew, in its order) -> (mat_in [B,6] f32, the matrix
    nn_ops.image_preprocess / cn_aug_image take, for the stored unflipped image with the flip folded in; trans_out [B,6] f64, the
    `trans_output` CenterNetTargets takes; flip_width [B] i32, w where the sample is flipped, else 0)."""
    dev = draws.device
    s, d = _sizes2("cn_aug_transform", sizes, dev), _f64c(draws, dev)
    B = s.shape[0]
    if d.dim() != 2 or d.shape != (B, 4):
        raise ValueError(f"cn_aug_transform: draws are [B, 4] float64, got {tuple(d.shape)} for B = {B}")
    at = _CNAugTransformAttrs(int(bool(rand_crop)), float(scale), float(shift), float(flip_prop), int(input_hw[0]), int(input_hw[1]), int(down_ratio))
    mat_in = torch.empty((B, 6), dtype=torch.float32, device=dev)
    trans_out = torch.empty((B, 6), dtype=torch.float64, device=dev)
    flip_width = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call("md_cn_aug_transform", [s, d, mat_in, trans_out, flip_width], extra=at)
    return mat_in, trans_out, flip_width


def cn_aug_image_workspace_bytes(B, out_h, out_w):
    """bytes of scratch md_cn_aug_image takes with colour augmentation (include/minddet_hip_cnaug.h)"""
    return _lib.workspace_bytes("md_cn_aug_image", B, out_h, out_w)


def cn_aug_image(img_u8, sizes, mat_in, mean, std, out_hw, colour=None, stem_layout=True, workspace=True, out=None):
    """cv2.warpAffine + / 255 + color_aug + (inp - mean) / std + the layout on the device (md_cn_aug_image): img_u8 [B,Hs,Ws,3] uint8
    BGR samples padded to a common extent, sizes [B,2] (h, w) of each, mat_in [B,6] f32, colour [B,8] f64 (three alphas, three
    lighting terms, the order index 0..5 of CN_COLOUR_ORDERS, one spare) or None -> the bf16 network input in the layout of
    nn_ops.image_preprocess (stem_layout: the zero-bordered 4-channel layout, else [B,out_h,out_w,8]).  colour None: the same bits as
    nn_ops.image_preprocess.  workspace=False leaves the scratch to the library's per-stream pool."""
    from .nn_ops import STEM_PAD_HI, STEM_PAD_LO

    dev, B = img_u8.device, img_u8.shape[0]
    ho, wo = (int(v) for v in out_hw)
    lo, hi, c = (STEM_PAD_LO, STEM_PAD_HI, 4) if stem_layout else (0, 0, 8)
    shape = (B, ho + lo + hi, wo + lo + hi, c)
    if out is None:
        out = torch.empty(shape, dtype=torch.bfloat16, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.bfloat16:
        raise ValueError(f"cn_aug_image: out is {shape} bfloat16")
    norm = torch.tensor([float(v) for v in mean] + [float(v) for v in std], dtype=torch.float32, device=dev)
    ops = [img_u8, _sizes2("cn_aug_image", sizes, dev), _f32c(mat_in), norm, None if colour is None else _f64c(colour, dev), out]
    if workspace and colour is not None:
        ops.append(_lib.scratch("md_cn_aug_image", (B, ho, wo), dev))
    _lib.call("md_cn_aug_image", ops, extra=_CNAugImageAttrs(ho, wo, lo, hi))
    return out


class CenterNetAugment:
    """The training branch of COCOHP.preprocess_fn in front of the targets (centernet/src/dataset.py:278-315, color_aug of
    centernet/src/image.py:208-253) on the device, built from the reference's dataset_config keys: rand_crop, scale, shift, flip_prop,
    color_aug, eig_val, eig_vec, mean, std, plus input_hw (input_res_train), down_ratio and stem_layout (None: the stem's 4-channel
    layout where nn_ops.stem_layout_ok(input_hw), else [B,H,W,8]).  color_aug's constants are the reference's
    (image.py:252-253: the three alphas 1 + U(-0.4, 0.4), the lighting alpha N(0, 0.1)).

    draw() makes the random values with the reference's distributions from torch's generator, NOT from numpy's and Python's random
    streams: the reference's distributions, not its sequence.

    Not built, a true / non-zero value raises ValueError: a rotation (rot, aug_rot, rotate), keep_res, and a down_ratio that differs
    between the two axes."""

    _ZERO_ONLY = ("rot", "aug_rot", "rotate", "keep_res")

    def __init__(self, input_hw=(512, 512), down_ratio=4, rand_crop=True, scale=0.4, shift=0.1, flip_prop=0.5, color_aug=True,
                 eig_val=(0.2141788, 0.01817699, 0.00341571),
                 eig_vec=((-0.58752847, -0.69563484, 0.41340352), (-0.5832747, 0.00994535, -0.81221408), (-0.56089297, 0.71832671, 0.41158938)),
                 mean=(0.40789654, 0.44719302, 0.47026115), std=(0.28863828, 0.27408164, 0.27809835), stem_layout=None, **options):
        for k, v in options.items():
            if k not in self._ZERO_ONLY:
                raise ValueError(f"CenterNetAugment: unknown option {k!r}")
            if v not in (None, False, 0, 0.0):
                raise ValueError(f"CenterNetAugment: {k} is not built")
        if isinstance(down_ratio, (list, tuple)):
            if len(set(int(v) for v in down_ratio)) != 1:
                raise ValueError("CenterNetAugment: a down_ratio that differs between the axes is not built")
            down_ratio = down_ratio[0]
        self.input_hw, self.down_ratio = (int(input_hw[0]), int(input_hw[1])), int(down_ratio)
        if min(self.input_hw) < self.down_ratio or self.down_ratio < 1:
            raise ValueError("CenterNetAugment: input_hw >= down_ratio >= 1")
        if stem_layout is None:            # the one-launch stem's layout wherever the input extent admits it (nn_ops.stem_layout_ok)
            from .nn_ops import stem_layout_ok
            stem_layout = stem_layout_ok(*self.input_hw)
        self.rand_crop, self.color_aug, self.stem_layout = bool(rand_crop), bool(color_aug), bool(stem_layout)
        self.scale, self.shift, self.flip_prop = float(scale), float(shift), float(flip_prop)
        if not 0.0 <= self.flip_prop <= 1.0:
            raise ValueError("CenterNetAugment: flip_prop in [0, 1]")
        # the reference holds the four arrays in fp32 (default_config.yaml:88-93)
        self.eig_val = np.asarray(eig_val, np.float32).astype(np.float64)
        self.eig_vec = np.asarray(eig_vec, np.float32).astype(np.float64)
        self.mean, self.std = tuple(np.asarray(mean, np.float32).tolist()), tuple(np.asarray(std, np.float32).tolist())
        if self.eig_val.shape != (3,) or self.eig_vec.shape != (3, 3) or len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError("CenterNetAugment: eig_val, mean, std have 3 values, eig_vec 3 x 3")

    @classmethod
    def from_config(cls, cfg):
        """cfg.train_cfg["augment"] (the reference's keys) on the input of cfg.train_cfg["assigner"] (input_res, down_ratio)"""
        a = cfg.train_cfg["assigner"]
        return cls(a["input_res"], a["down_ratio"], **dict(cfg.train_cfg["augment"]))

    @staticmethod
    def get_border(border, size):
        """COCOHP._get_border (dataset.py:207-211) as tensor arithmetic: border // i for the first i = 1, 2, 4, ... with
        size - border // i > border // i"""
        out, found = torch.zeros_like(size), torch.zeros_like(size, dtype=torch.bool)
        i = 1
        while True:
            b = border // i
            ok = (size - b > b) & ~found
            out = torch.where(ok, torch.full_like(size, b), out)
            found = found | ok
            if b == 0:
                return out
            i *= 2

    def draw(self, sizes, generator=None):
        """sizes [B,2] (h, w) on the device -> (draws [B,4] f64, colour [B,8] f64 or None without color_aug), the operands of
        cn_aug_transform / cn_aug_image, with the reference's distributions.  rand_crop: np.random.choice(np.arange(0.6, 1.4, 0.1)) as
        element i of that array with i uniform in 0..7, np.random.randint(border, size - border) per axis with _get_border(128, size); else three
        standard normals; the flip's uniform; colour: 1 + U(-0.4, 0.4) three times, eig_vec . (eig_val * N(0, 0.1)^3), the order uniform
        over the six permutations.  Nothing is read back."""
        s = sizes if generator is None else sizes.to(generator.device)
        dev, B = s.device, s.shape[0]
        f64 = dict(dtype=torch.float64, device=dev, generator=generator)
        draws = torch.empty((B, 4), dtype=torch.float64, device=dev)
        if self.rand_crop:
            table = torch.as_tensor(np.arange(0.6, 1.4, 0.1), device=dev)      # np.arange's own eight values
            draws[:, 0] = table[torch.floor(torch.rand((B,), **f64) * 8).clamp_(max=7).long()]
            for col, k in ((1, 1), (2, 0)):             # c[0] along the width, c[1] along the height
                size = s[:, k].to(torch.int64)
                lo = self.get_border(128, size)
                span = (size - 2 * lo).clamp(min=1).to(torch.float64)
                off = torch.minimum(torch.floor(torch.rand((B,), **f64) * span), span - 1)
                draws[:, col] = lo.to(torch.float64) + off
        else:
            draws[:, :3] = torch.randn((B, 3), **f64)
        draws[:, 3] = torch.rand((B,), **f64)
        if not self.color_aug:
            return draws, None
        colour = torch.zeros((B, 8), dtype=torch.float64, device=dev)
        colour[:, :3] = 1.0 + (torch.rand((B, 3), **f64) * 0.8 - 0.4)
        alpha = torch.randn((B, 3), **f64) * 0.1
        val = torch.as_tensor(self.eig_val, device=dev)
        vec = torch.as_tensor(self.eig_vec, device=dev)
        colour[:, 3:6] = (alpha * val) @ vec.T
        colour[:, 6] = torch.floor(torch.rand((B,), **f64) * 6).clamp_(max=5)
        return draws, colour

    def __call__(self, images_u8, sizes, draws=None, colour=None, generator=None):
        """images_u8 [B,Hs,Ws,3] uint8 BGR on the device (padded to a common extent), sizes [B,2] (h, w); draws / colour: the pair of
        draw() (None: drawn here with `generator`; color_aug False: no colour is applied) -> (input: the bf16 network input, trans_out
        [B,6] f64, flip_width [B] i32), nothing read back."""
        dev = images_u8.device
        s = _sizes2("CenterNetAugment", sizes, dev)
        if draws is None:
            draws, drawn = self.draw(s, generator)
            colour = drawn if colour is None else colour
        if not self.color_aug:
            colour = None
        elif colour is None:
            colour = self.draw(s, generator)[1]
        mat_in, trans_out, flip_width = cn_aug_transform(s, draws.to(dev), rand_crop=self.rand_crop, scale=self.scale, shift=self.shift,
                                                         flip_prop=self.flip_prop, input_hw=self.input_hw, down_ratio=self.down_ratio)
        inp = cn_aug_image(images_u8, s, mat_in, self.mean, self.std, self.input_hw, colour=colour, stem_layout=self.stem_layout)
        return inp, trans_out, flip_width


# ----------------------------------------------------------------------------- KITTI camera-frame ends (csrc/kitti.hip)
CROP_MAX_HULLS, CROP_MAX_BATCH = 64, 4096                          # MD_CROP_MAX_HULLS, MD_CROP_MAX_BATCH
KITTI_MAX_DETS, KITTI_MAX_LABELS, KITTI_MAX_BATCH = 512, 4096, 4096     # MD_KITTI_MAX_DETS, MD_KITTI_MAX_LABELS, MD_KITTI_MAX_BATCH
_KITTI_REFUSED = ("remove_environment", "random_crop", "generate_single_sample_dict", "fp32_calibration")


class _KittiRowsAttrs(ctypes.Structure):
    _fields_ = [("limit_range", ctypes.c_float * 6), ("use_limit", ctypes.c_int32), ("lidar_input", ctypes.c_int32)]


def kitti_io_options(**options):
    """The options of prep_pointcloud / predict.py that the KITTI device chain does not build: a true value raises ValueError.
    remove_environment (the reference calls it on boxes that are still in the camera frame, data/preprocess.py:79 before :87: a quirk
    nobody should want restated), random_crop, generate_single_sample_dict (use_self_train=False) and fp32 calibration arithmetic."""
    for k, v in options.items():
        if k == "use_self_train":
            if v is False:
                raise ValueError("kitti: generate_single_sample_dict (use_self_train=False) is not built")
        elif k not in _KITTI_REFUSED:
            raise ValueError(f"kitti: unknown option {k!r}")
        elif v not in (None, False):
            raise ValueError(f"kitti: {k} is not built")


def _crt_kitti(proj):
    """projection_matrix_to_crt_kitti (box_np_ops.py:395-408), the same numpy calls"""
    cr, ct = proj[0:3, 0:3], proj[0:3, 3]
    rinv, cinv = np.linalg.qr(np.linalg.inv(cr))
    return np.linalg.inv(cinv), np.linalg.inv(rinv), cinv @ ct


def _frustum_corners(bboxes, c, near_clip=0.001, far_clip=100):
    """get_frustum_v2 (box_np_ops.py:432-449; get_frustum :410-428 is its one-box form): bboxes [n,4] -> [n,8,3] in the camera frame"""
    fku, fkv, u0v0 = c[0, 0], -c[1, 1], c[0:2, 2]
    n = bboxes.shape[0]
    z = np.tile(np.array([near_clip] * 4 + [far_clip] * 4, dtype=c.dtype)[np.newaxis, :, np.newaxis], [n, 1, 1])
    corners = bboxes[..., [0, 1, 0, 3, 2, 3, 2, 1]].reshape(-1, 4, 2)
    near = (corners - u0v0) / np.array([fku / near_clip, -fkv / near_clip], dtype=c.dtype)
    far = (corners - u0v0) / np.array([fku / far_clip, -fkv / far_clip], dtype=c.dtype)
    return np.concatenate([np.concatenate([near, far], axis=1), z], axis=-1)


class KittiCalibration:
    """The calibration of a batch of KITTI frames and its products, composed on the host in float64 and uploaded once each:
    rect [B,4,4] (R0_rect), trv2c [B,4,4] (Tr_velo_to_cam), p2 [B,4,4], image_shape [B,2] (h, w).  A single frame may come without the
    batch axis.  The arrays are widened to float64 -- a stated choice: the reference works in the calibration arrays' dtype (fp32 in its
    info files); fp32_calibration=True is refused.
      lidar2cam   rect @ trv2c                           (lidar_to_camera, box_np_ops.py:590-596)
      cam2lidar   inv(rect @ trv2c)                      (camera_to_lidar multiplies by inv((rect @ trv2c).T) from the right, :581-587)
      image_frustum()            [B,1,8,3] lidar-frame corners of remove_outside_points (:625-632): projection_matrix_to_crt_kitti,
                                 get_frustum of [0, 0, w, h], -= t, inv(r) @, camera_to_lidar -- the same numpy calls
      detection_frustums(bboxes [B,K,4], count)   (hulls [B,K,8,3], count) of the reference_detections lines (data/preprocess.py:59-65)
    device: where tensor() puts the products ("cpu" keeps everything on the host, for tests without a GPU)."""

    def __init__(self, rect, trv2c, p2, image_shape, device="cuda", **options):
        kitti_io_options(**options)

        def mats(a, name):
            a = np.asarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
            a = a[None] if a.ndim == 2 else a
            if a.ndim != 3 or a.shape[1:] != (4, 4):
                raise ValueError(f"KittiCalibration: {name} is [B, 4, 4] (KITTI's 3x4 extended by the row 0 0 0 1), got {a.shape}")
            return np.ascontiguousarray(a)

        self.rect, self.trv2c, self.p2 = mats(rect, "rect"), mats(trv2c, "trv2c"), mats(p2, "p2")
        shp = np.asarray(image_shape.cpu().numpy() if isinstance(image_shape, torch.Tensor) else image_shape)
        shp = shp[None] if shp.ndim == 1 else shp
        self.B = len(self.rect)
        if shp.shape != (self.B, 2) or len(self.trv2c) != self.B or len(self.p2) != self.B:
            raise ValueError("KittiCalibration: rect, trv2c and p2 are [B, 4, 4] and image_shape [B, 2] (h, w) for one B")
        if self.B > KITTI_MAX_BATCH:
            raise ValueError(f"KittiCalibration: at most {KITTI_MAX_BATCH} frames")
        self.image_shape = np.ascontiguousarray(shp, dtype=np.int32)
        self.device = device
        self.lidar2cam = np.stack([r @ t for r, t in zip(self.rect, self.trv2c)])
        self.cam2lidar = np.stack([np.linalg.inv(m) for m in self.lidar2cam])
        self._crt = [_crt_kitti(p) for p in self.p2]
        self._dev = {}

    def _to_lidar(self, b, frustums):
        """frustums [n,8,3] in the camera frame of P2 -> the lidar frame, as remove_outside_points and prep_pointcloud do"""
        _, r, t = self._crt[b]
        f = frustums - t
        f = np.einsum("ij, akj->aki", np.linalg.inv(r), f)
        f = np.concatenate([f, np.ones(list(f.shape[:-1]) + [1])], axis=-1)
        return (f @ np.linalg.inv((self.rect[b] @ self.trv2c[b]).T))[..., :3]

    def image_frustum_host(self):
        out = []
        for b in range(self.B):
            h, w = self.image_shape[b]
            out.append(self._to_lidar(b, _frustum_corners(np.array([[0, 0, w, h]], dtype=np.float64), self._crt[b][0])))
        return np.stack(out) if out else np.zeros((0, 1, 8, 3))

    def detection_frustums_host(self, bboxes, count=None):
        bboxes = np.asarray(bboxes.cpu().numpy() if isinstance(bboxes, torch.Tensor) else bboxes, dtype=np.float64)
        if bboxes.ndim != 3 or bboxes.shape[0] != self.B or bboxes.shape[2] != 4:
            raise ValueError(f"KittiCalibration: reference detections are [B, K, 4] image boxes, got {bboxes.shape}")
        K = bboxes.shape[1]
        if K > CROP_MAX_HULLS:
            raise ValueError(f"KittiCalibration: at most {CROP_MAX_HULLS} reference detections per frame, got {K}")
        count = np.full(self.B, K, np.int32) if count is None else np.asarray(count.cpu().numpy() if isinstance(count, torch.Tensor) else count, np.int32)
        hulls = np.stack([self._to_lidar(b, _frustum_corners(bboxes[b], self._crt[b][0])) for b in range(self.B)]) if self.B and K else \
            np.zeros((self.B, K, 8, 3))
        return hulls, count

    def tensor(self, name):
        """lidar2cam, cam2lidar, p2, image_shape, image_frustum, image_count on the device, uploaded at the first use"""
        if name not in self._dev:
            host = {"image_frustum": self.image_frustum_host, "image_count": lambda: np.ones(self.B, np.int32)}.get(name, lambda: getattr(self, name))()
            self._dev[name] = torch.from_numpy(np.ascontiguousarray(host)).to(self.device)
        return self._dev[name]

    def image_frustum(self):
        return self.tensor("image_frustum")

    def detection_frustums(self, bboxes, count=None):
        hulls, count = self.detection_frustums_host(bboxes, count)
        return torch.from_numpy(np.ascontiguousarray(hulls)).to(self.device), torch.from_numpy(count).to(self.device)


def crop_hulls_workspace_bytes(N, B, K):
    """bytes of scratch md_pc_crop_hulls takes (include/minddet_hip_kitti.h)"""
    return _lib.workspace_bytes("md_pc_crop_hulls", N, B, K)


def crop_hulls(points, offsets, hulls, hull_count, workspace=True, out=None):
    """Keep the points inside any of a sample's convex hexahedra (md_pc_crop_hulls, include/minddet_hip_kitti.h): points [N,4] f32 with
    offsets [B+1] i32, hulls [B,K,8,3] f64 (lidar-frame corners in the reference's corner order), hull_count [B] i32 ->
    (points_out [N,4] f32 with zero rows behind the last kept row, offsets_out [B+1] i32, keep [N] u8).  out: an [N,4] f32 tensor to
    write into.  workspace=False leaves the scratch to the per-stream pool."""
    if points.dim() != 2 or points.shape[1] != 4:
        raise ValueError(f"crop_hulls: points are [N, 4] (other widths are not built), got {tuple(points.shape)}")
    points = _f32c(points)
    dev, N = points.device, points.shape[0]
    if hulls.dim() != 4 or tuple(hulls.shape[2:]) != (8, 3):
        raise ValueError(f"crop_hulls: hulls are [B, K, 8, 3], got {tuple(hulls.shape)}")
    B, K = hulls.shape[:2]
    if K > CROP_MAX_HULLS or B > CROP_MAX_BATCH:
        raise ValueError(f"crop_hulls: at most {CROP_MAX_HULLS} hulls per sample and {CROP_MAX_BATCH} samples, got {K} and {B}")
    if tuple(offsets.shape) != (B + 1,) or tuple(hull_count.shape) != (B,):
        raise ValueError(f"crop_hulls: offsets are [{B + 1}] and hull_count [{B}] beside hulls {tuple(hulls.shape)}")
    if out is None:
        out = torch.empty((N, 4), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (N, 4) or out.dtype != torch.float32:
        raise ValueError(f"crop_hulls: out is [{N}, 4] f32, got {tuple(out.shape)} {out.dtype}")
    offsets_out = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    keep = torch.empty((N,), dtype=torch.uint8, device=dev)
    ops = [points, _i32c(offsets, dev), _f64c(hulls, dev), _i32c(hull_count, dev), out, offsets_out, keep]
    if workspace:
        ops.append(_lib.scratch("md_pc_crop_hulls", (N, B, K), dev))
    _lib.call("md_pc_crop_hulls", ops)
    return out, offsets_out, keep


def kitti_boxes_to_lidar(boxes_cam, gt_count, cam2lidar):
    """box_camera_to_lidar for a batch (md_kitti_boxes_to_lidar): boxes_cam [B,G,7] f32 (x, y, z, l, h, w, r), gt_count [B],
    cam2lidar [B,4,4] f64 -> boxes_lidar [B,G,7] f32 (x, y, z, w, l, h, r), zero rows from the count on."""
    g = _f32c(boxes_cam)
    if g.dim() != 3 or g.shape[2] != 7:
        raise ValueError(f"kitti_boxes_to_lidar: boxes are [B, G, 7], got {tuple(g.shape)}")
    dev, (B, G) = g.device, g.shape[:2]
    if G > KITTI_MAX_LABELS or B > KITTI_MAX_BATCH:
        raise ValueError(f"kitti_boxes_to_lidar: at most {KITTI_MAX_LABELS} rows per sample and {KITTI_MAX_BATCH} samples")
    if tuple(cam2lidar.shape) != (B, 4, 4) or tuple(gt_count.shape) != (B,):
        raise ValueError(f"kitti_boxes_to_lidar: cam2lidar is [{B}, 4, 4] and gt_count [{B}]")
    out = torch.empty((B, G, 7), dtype=torch.float32, device=dev)
    _lib.call("md_kitti_boxes_to_lidar", [g, _i32c(gt_count, dev), _f64c(cam2lidar, dev), out])
    return out


def kitti_rows(dets, count, lidar2cam, p2, image_shape, limit_range=None, lidar_input=False):
    """generate_single_sample_dict_old (without its direction flip) + predict_kitti_to_anno for a batch (md_kitti_rows): dets [B,M,9] f32
    and count [B] as the KITTI model's forward returns them, lidar2cam / p2 [B,4,4] f64, image_shape [B,2] i32 (h, w); limit_range =
    post_center_limit_range or None -> (rows [B,M,14] f32: alpha, bbox, dimensions l h w, location, rotation_y, score, label;
    src [B,M] i32; out_count [B] i32)."""
    d = _f32c(dets)
    if d.dim() != 3 or d.shape[2] != 9:
        raise ValueError(f"kitti_rows: dets are [B, M, 9], got {tuple(d.shape)}")
    dev, (B, M) = d.device, d.shape[:2]
    if M > KITTI_MAX_DETS or B > KITTI_MAX_BATCH:
        raise ValueError(f"kitti_rows: at most {KITTI_MAX_DETS} detections per sample and {KITTI_MAX_BATCH} samples")
    for name, t, want in (("count", count, (B,)), ("lidar2cam", lidar2cam, (B, 4, 4)), ("p2", p2, (B, 4, 4)), ("image_shape", image_shape, (B, 2))):
        if tuple(t.shape) != want:
            raise ValueError(f"kitti_rows: {name} is {list(want)}, got {tuple(t.shape)}")
    lim = [0.0] * 6 if limit_range is None else [float(v) for v in limit_range]
    if len(lim) != 6 or any(math.isnan(v) for v in lim):
        raise ValueError("kitti_rows: limit_range has six values, none a NaN")
    at = _KittiRowsAttrs((ctypes.c_float * 6)(*lim), int(limit_range is not None), int(bool(lidar_input)))
    rows = torch.empty((B, M, 14), dtype=torch.float32, device=dev)
    src = torch.empty((B, M), dtype=torch.int32, device=dev)
    out_count = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call("md_kitti_rows", [d, _i32c(count, dev), _f64c(lidar2cam, dev), _f64c(p2, dev), _i32c(image_shape, dev), rows, src, out_count], extra=at)
    return rows, src, out_count


# ----------------------------------------------------------------------------- KITTI AP evaluation (csrc/kittieval.hip)
KEVAL_MAX_DETS, KEVAL_MAX_GTS, KEVAL_MAX_IMAGES = 512, 512, 65536      # MD_KEVAL_MAX_DETS, MD_KEVAL_MAX_GTS, MD_KEVAL_MAX_IMAGES
KEVAL_MAX_CLASSES, KEVAL_MAX_LEVELS, KEVAL_SAMPLE_PTS = 8, 4, 41       # MD_KEVAL_MAX_CLASSES, MD_KEVAL_MAX_LEVELS, MD_KEVAL_SAMPLE_PTS


class _KittiEvalFlagsAttrs(ctypes.Structure):
    _fields_ = [("abs_gt_height", ctypes.c_int32)]


class _KittiEvalOverlapsAttrs(ctypes.Structure):
    _fields_ = [("metric", ctypes.c_int32)]


class _KittiEvalStatsAttrs(ctypes.Structure):
    _fields_ = [("metric", ctypes.c_int32), ("compute_aos", ctypes.c_int32)]


def _i64c(t, dev):
    return t.to(device=dev, dtype=torch.int64).contiguous()


def _keval_shape(who, name, t, want):
    if tuple(t.shape) != tuple(want):
        raise ValueError(f"{who}: {name} is {list(want)}, got {tuple(t.shape)}")


def _keval_limits(who, I=0, Cn=1, K=1, Gt=0, Dt=0, P=0):
    if Cn < 1 or K < 1:
        raise ValueError(f"{who}: at least one class and one overlap level")
    if I > KEVAL_MAX_IMAGES or Cn > KEVAL_MAX_CLASSES or K > KEVAL_MAX_LEVELS:
        raise ValueError(f"{who}: at most {KEVAL_MAX_IMAGES} images, {KEVAL_MAX_CLASSES} classes and {KEVAL_MAX_LEVELS} overlap levels, got {I}, {Cn}, {K}")
    if Gt > KEVAL_MAX_IMAGES * KEVAL_MAX_GTS or Dt > KEVAL_MAX_IMAGES * KEVAL_MAX_DETS or P >= 1 << 31:
        raise ValueError(f"{who}: at most {KEVAL_MAX_GTS} ground truths and {KEVAL_MAX_DETS} detections per image and fewer than 2^31 pairs")


def kitti_eval_flags(gt_box, gt_occ, gt_trunc, gt_valid, dt_box, dt_same, abs_gt_height=False):
    """clean_data for the three difficulties and the Cn classes of gt_valid / dt_same (md_kitti_eval_flags, include/
    minddet_hip_kittieval.h): gt_box [Gt,4] f64, gt_occ [Gt] i32, gt_trunc [Gt] f64, gt_valid [Cn,Gt] u8, dt_box [Dt,4] f64,
    dt_same [Cn,Dt] u8 -> (ign_gt [Cn,3,Gt] u8, ign_dt [Cn,3,Dt] u8, num_valid [Cn,3] i32); the flags as 1 + clean_data's."""
    who, dev = "kitti_eval_flags", gt_box.device
    if gt_box.dim() != 2 or gt_box.shape[1] != 4 or dt_box.dim() != 2 or dt_box.shape[1] != 4 or gt_valid.dim() != 2:
        raise ValueError(f"{who}: gt_box is [Gt, 4], dt_box [Dt, 4] and gt_valid [Cn, Gt]")
    Gt, Dt, Cn = gt_box.shape[0], dt_box.shape[0], gt_valid.shape[0]
    for name, t, want in (("gt_occ", gt_occ, (Gt,)), ("gt_trunc", gt_trunc, (Gt,)), ("gt_valid", gt_valid, (Cn, Gt)), ("dt_same", dt_same, (Cn, Dt))):
        _keval_shape(who, name, t, want)
    _keval_limits(who, Cn=Cn, Gt=Gt, Dt=Dt)
    ign_gt = torch.empty((Cn, 3, Gt), dtype=torch.uint8, device=dev)
    ign_dt = torch.empty((Cn, 3, Dt), dtype=torch.uint8, device=dev)
    num_valid = torch.empty((Cn, 3), dtype=torch.int32, device=dev)
    _lib.call("md_kitti_eval_flags", [_f64c(gt_box, dev), _i32c(gt_occ, dev), _f64c(gt_trunc, dev), _u8c(gt_valid, dev), _f64c(dt_box, dev),
                                      _u8c(dt_same, dev), ign_gt, ign_dt, num_valid], extra=_KittiEvalFlagsAttrs(int(bool(abs_gt_height))))
    return ign_gt, ign_dt, num_valid


def kitti_eval_overlaps(gt_off, dt_off, ov_off, gt, dt, metric, pairs):
    """calculate_overlaps for all images in one launch (md_kitti_eval_overlaps): offsets [I+1] (ov_off i64), gt / dt the image boxes
    [.,4] f64 for metric 0, the camera boxes [.,7] f64 for metrics 1 and 2; pairs: the length of the result, at least ov_off[I] (the
    host knows it from the extents) -> ov [pairs] f64, image i's block ground-truth-major [G_i, D_i] at ov_off[i]."""
    who, dev = "kitti_eval_overlaps", gt.device
    if metric not in (0, 1, 2):
        raise ValueError(f"{who}: metric is 0, 1 or 2, got {metric!r}")
    W = 4 if metric == 0 else 7
    if gt.dim() != 2 or gt.shape[1] != W or dt.dim() != 2 or dt.shape[1] != W or gt_off.dim() != 1 or gt_off.shape[0] < 1:
        raise ValueError(f"{who}: metric {metric} takes gt [Gt, {W}] and dt [Dt, {W}] and offsets [I + 1]")
    I = gt_off.shape[0] - 1
    _keval_shape(who, "dt_off", dt_off, (I + 1,))
    _keval_shape(who, "ov_off", ov_off, (I + 1,))
    _keval_limits(who, I=I, Gt=gt.shape[0], Dt=dt.shape[0], P=int(pairs))
    ov = torch.empty((int(pairs),), dtype=torch.float64, device=dev)
    _lib.call("md_kitti_eval_overlaps", [_i32c(gt_off, dev), _i32c(dt_off, dev), _i64c(ov_off, dev), _f64c(gt, dev), _f64c(dt, dev), ov],
              extra=_KittiEvalOverlapsAttrs(int(metric)))
    return ov


def _keval_match_operands(who, ov, ign_gt, ign_dt, dt_score, gt_off, dt_off, ov_off, min_overlap):
    if ov.dim() != 1 or ign_gt.dim() != 3 or ign_dt.dim() != 3 or ign_gt.shape[1] != 3 or min_overlap.dim() != 2 or gt_off.dim() != 1 or gt_off.shape[0] < 1:
        raise ValueError(f"{who}: ov is [P], ign_gt [Cn, 3, Gt], ign_dt [Cn, 3, Dt], min_overlap [Cn, K] and the offsets [I + 1]")
    dev, (Cn, _, Gt), Dt, I, K = ov.device, ign_gt.shape, ign_dt.shape[2], gt_off.shape[0] - 1, min_overlap.shape[1]
    for name, t, want in (("ign_dt", ign_dt, (Cn, 3, Dt)), ("dt_score", dt_score, (Dt,)), ("dt_off", dt_off, (I + 1,)), ("ov_off", ov_off, (I + 1,)),
                          ("min_overlap", min_overlap, (Cn, K))):
        _keval_shape(who, name, t, want)
    _keval_limits(who, I=I, Cn=Cn, K=K, Gt=Gt, Dt=Dt, P=ov.shape[0])
    ops = [_f64c(ov, dev), _u8c(ign_gt, dev), _u8c(ign_dt, dev), _f64c(dt_score, dev), _i32c(gt_off, dev), _i32c(dt_off, dev), _i64c(ov_off, dev),
           _f64c(min_overlap, dev)]
    return ops, dev, I, Cn, K, Gt, Dt


def kitti_eval_match(ov, ign_gt, ign_dt, dt_score, gt_off, dt_off, ov_off, min_overlap):
    """Pass 1 of eval_class for every (class, difficulty, overlap level, image) (md_kitti_eval_match) -> matched [Cn,3,K,Gt] f64: the
    score of the detection that became a true positive for the ground truth, -inf otherwise."""
    ops, dev, I, Cn, K, Gt, Dt = _keval_match_operands("kitti_eval_match", ov, ign_gt, ign_dt, dt_score, gt_off, dt_off, ov_off, min_overlap)
    matched = torch.empty((Cn, 3, K, Gt), dtype=torch.float64, device=dev)
    _lib.call("md_kitti_eval_match", ops + [matched])
    return matched


def kitti_eval_thresholds(sorted_scores, num_valid):
    """get_thresholds for every task (md_kitti_eval_thresholds): sorted_scores [Cn,3,K,Gt] f64, the rows of kitti_eval_match's result
    sorted descending; num_valid [Cn,3] i32 -> (thresholds [Cn,3,K,41] f64, NaN behind nthresh; nthresh [Cn,3,K] i32)."""
    who, dev = "kitti_eval_thresholds", sorted_scores.device
    if sorted_scores.dim() != 4 or sorted_scores.shape[1] != 3:
        raise ValueError(f"{who}: the scores are [Cn, 3, K, Gt], got {tuple(sorted_scores.shape)}")
    Cn, _, K, Gt = sorted_scores.shape
    _keval_shape(who, "num_valid", num_valid, (Cn, 3))
    _keval_limits(who, Cn=Cn, K=K, Gt=Gt)
    thresholds = torch.empty((Cn, 3, K, KEVAL_SAMPLE_PTS), dtype=torch.float64, device=dev)
    nthresh = torch.empty((Cn, 3, K), dtype=torch.int32, device=dev)
    _lib.call("md_kitti_eval_thresholds", [_f64c(sorted_scores, dev), _i32c(num_valid, dev), thresholds, nthresh])
    return thresholds, nthresh


def kitti_eval_stats(ov, ign_gt, ign_dt, dt_score, gt_off, dt_off, ov_off, min_overlap, thresholds, nthresh, gt_box, gt_dc, dt_box, gt_alpha,
                     dt_alpha, metric, compute_aos=False):
    """Pass 2 of eval_class for every (task, threshold, image) and the sums over the images (md_kitti_eval_stats) -> (img_counts
    [Cn,3,K,41,I,3] i32 (tp, fp, fn), img_sim [Cn,3,K,41,I] f64, pr_counts [Cn,3,K,41,3] i32, pr_sim [Cn,3,K,41] f64); rows at or
    behind nthresh are zero."""
    who = "kitti_eval_stats"
    if metric not in (0, 1, 2):
        raise ValueError(f"{who}: metric is 0, 1 or 2, got {metric!r}")
    ops, dev, I, Cn, K, Gt, Dt = _keval_match_operands(who, ov, ign_gt, ign_dt, dt_score, gt_off, dt_off, ov_off, min_overlap)
    N = KEVAL_SAMPLE_PTS
    for name, t, want in (("thresholds", thresholds, (Cn, 3, K, N)), ("nthresh", nthresh, (Cn, 3, K)), ("gt_box", gt_box, (Gt, 4)), ("gt_dc", gt_dc, (Gt,)),
                          ("dt_box", dt_box, (Dt, 4)), ("gt_alpha", gt_alpha, (Gt,)), ("dt_alpha", dt_alpha, (Dt,))):
        _keval_shape(who, name, t, want)
    img_counts = torch.empty((Cn, 3, K, N, I, 3), dtype=torch.int32, device=dev)
    img_sim = torch.empty((Cn, 3, K, N, I), dtype=torch.float64, device=dev)
    pr_counts = torch.empty((Cn, 3, K, N, 3), dtype=torch.int32, device=dev)
    pr_sim = torch.empty((Cn, 3, K, N), dtype=torch.float64, device=dev)
    ops += [_f64c(thresholds, dev), _i32c(nthresh, dev), _f64c(gt_box, dev), _u8c(gt_dc, dev), _f64c(dt_box, dev), _f64c(gt_alpha, dev),
            _f64c(dt_alpha, dev), img_counts, img_sim, pr_counts, pr_sim]
    _lib.call("md_kitti_eval_stats", ops, extra=_KittiEvalStatsAttrs(int(metric), int(bool(compute_aos))))
    return img_counts, img_sim, pr_counts, pr_sim


# ----------------------------------------------------------------------------- COCO bbox AP evaluation (csrc/cocoeval.hip)
COCOEVAL_MAX_DETS, COCOEVAL_MAX_GTS, COCOEVAL_MAX_IMAGE_DETS = 100, 256, 512      # MD_COCOEVAL_MAX_DETS, _MAX_GTS, _MAX_IMAGE_DETS
COCOEVAL_MAX_CELLS, COCOEVAL_MAX_CATS, COCOEVAL_MAX_ROWS = 1 << 24, 128, 1 << 26   # MD_COCOEVAL_MAX_CELLS, _MAX_CATS, _MAX_ROWS
COCOEVAL_MAX_LABELS, COCOEVAL_MAX_THRS, COCOEVAL_MAX_AREAS = 4096, 16, 8           # MD_COCOEVAL_MAX_LABELS, _MAX_THRS, _MAX_AREAS
COCOEVAL_MAX_RECS, COCOEVAL_MAX_MAXDETS = 256, 8                                   # MD_COCOEVAL_MAX_RECS, _MAX_MAXDETS


class _CocoEvalRowsAttrs(ctypes.Structure):
    _fields_ = [("first_image", ctypes.c_int32)]


def _ceval_limits(who, C=1, Kc=1, Gt=0, Dt=0, T=1, A=1, R=1, M=1):
    if min(C, Kc, T, A, R, M) < 1:
        raise ValueError(f"{who}: at least one cell, category, threshold, area range, recall threshold and maxDets value")
    if C >= COCOEVAL_MAX_CELLS or Kc > COCOEVAL_MAX_CATS or Gt > COCOEVAL_MAX_ROWS or Dt > COCOEVAL_MAX_ROWS:
        raise ValueError(f"{who}: fewer than {COCOEVAL_MAX_CELLS} cells, at most {COCOEVAL_MAX_CATS} categories and {COCOEVAL_MAX_ROWS} rows, got "
                         f"{C}, {Kc}, {max(Gt, Dt)}")
    if T > COCOEVAL_MAX_THRS or A > COCOEVAL_MAX_AREAS or R > COCOEVAL_MAX_RECS or M > COCOEVAL_MAX_MAXDETS or A * T * Dt >= 1 << 31:
        raise ValueError(f"{who}: at most {COCOEVAL_MAX_THRS} IoU thresholds, {COCOEVAL_MAX_AREAS} area ranges, {COCOEVAL_MAX_RECS} recall thresholds, "
                         f"{COCOEVAL_MAX_MAXDETS} maxDets values and fewer than 2^31 (area range, threshold, row) entries")


def coco_eval_rows(dets, count, label_to_k, first_image, dt_box, dt_area, dt_score, dt_cat, dt_rank, dt_beg, dt_cnt, dt_src):
    """dets_to_coco + the grouping into (image, category) cells for one batch, nothing read back (md_coco_eval_rows, include/
    minddet_hip_cocoeval.h): dets [B,max_det,6] f32 (x1, y1, x2, y2, score, label), count [B] i32, label_to_k [L] i32 (-1 drops the row).
    The eight outputs are the operands of the whole set (Dt = I max_det rows, I Kc cells), written in place for the images
    first_image .. first_image + B - 1: dt_box [Dt,4] f64, dt_area, dt_score [Dt] f64, dt_cat, dt_rank [Dt] i32, dt_beg, dt_cnt [I Kc]
    i32, dt_src [Dt] i32."""
    who = "coco_eval_rows"
    if dets.dim() != 3 or dets.shape[2] != 6 or dets.shape[1] < 1 or dets.dtype != torch.float32:
        raise ValueError(f"{who}: dets are [B, max_det, 6] float32, got {tuple(dets.shape)} {dets.dtype}")
    dev, (B, max_det) = dets.device, dets.shape[:2]
    if max_det > COCOEVAL_MAX_IMAGE_DETS:
        raise ValueError(f"{who}: at most {COCOEVAL_MAX_IMAGE_DETS} rows per image, got {max_det}")
    if label_to_k.dim() != 1 or not 1 <= label_to_k.shape[0] <= COCOEVAL_MAX_LABELS:
        raise ValueError(f"{who}: label_to_k is [L], 1 <= L <= {COCOEVAL_MAX_LABELS}")
    _keval_shape(who, "count", count, (B,))
    if dt_box.dim() != 2 or dt_beg.dim() != 1 or dt_box.shape[0] < 1 or dt_box.shape[0] % max_det or dt_beg.shape[0] < 1:
        raise ValueError(f"{who}: dt_box is [I max_det, 4] and dt_beg [I Kc]")
    Dt, C = dt_box.shape[0], dt_beg.shape[0]
    I = Dt // max_det
    if C % I:
        raise ValueError(f"{who}: {C} cells are no multiple of {I} images")
    outs = (("dt_box", dt_box, (Dt, 4), torch.float64), ("dt_area", dt_area, (Dt,), torch.float64), ("dt_score", dt_score, (Dt,), torch.float64),
            ("dt_cat", dt_cat, (Dt,), torch.int32), ("dt_rank", dt_rank, (Dt,), torch.int32), ("dt_beg", dt_beg, (C,), torch.int32),
            ("dt_cnt", dt_cnt, (C,), torch.int32), ("dt_src", dt_src, (Dt,), torch.int32))
    for name, t, want, dtype in outs:
        _keval_shape(who, name, t, want)
        if t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{who}: {name} is a contiguous {dtype} tensor on {dev} (it is written in place)")
    _ceval_limits(who, C=C, Kc=C // I, Dt=Dt)
    if first_image < 0 or first_image + B > I:
        raise ValueError(f"{who}: images {first_image} .. {first_image + B - 1} of {I}")
    _lib.call("md_coco_eval_rows", [dets.contiguous(), _i32c(count, dev), _i32c(label_to_k, dev)] + [t for _, t, _, _ in outs],
              extra=_CocoEvalRowsAttrs(int(first_image)))


def coco_eval_match(gt_beg, gt_cnt, dt_beg, dt_cnt, gt_box, gt_area, gt_crowd, gt_ignore, dt_box, dt_area, iou_thr, area_rng):
    """COCOBboxEval._evaluate_img for every (cell, area range) and all thresholds (md_coco_eval_match): the cell tables [I Kc] i32, the
    ground-truth rows (gt_box [Gt,4], gt_area [Gt] f64, gt_crowd, gt_ignore [Gt] u8), the detection rows (dt_box [Dt,4], dt_area [Dt]
    f64), iou_thr [T] f64, area_rng [A,2] f64 -> (dtm [A,T,Dt] i32: the packed ground-truth row matched or -1, dt_ig [A,T,Dt] u8,
    cell_ngt [A, I Kc] i32).  The per-cell counts are device data the kernel clamps; the packer refuses a cell beyond the limits."""
    who, dev = "coco_eval_match", gt_box.device
    if gt_beg.dim() != 1 or gt_box.dim() != 2 or gt_box.shape[1] != 4 or dt_box.dim() != 2 or dt_box.shape[1] != 4 or iou_thr.dim() != 1 or area_rng.dim() != 2:
        raise ValueError(f"{who}: the cell tables are [I Kc], gt_box [Gt, 4], dt_box [Dt, 4], iou_thr [T] and area_rng [A, 2]")
    C, Gt, Dt, T, A = gt_beg.shape[0], gt_box.shape[0], dt_box.shape[0], iou_thr.shape[0], area_rng.shape[0]
    for name, t, want in (("gt_cnt", gt_cnt, (C,)), ("dt_beg", dt_beg, (C,)), ("dt_cnt", dt_cnt, (C,)), ("gt_area", gt_area, (Gt,)), ("gt_crowd", gt_crowd, (Gt,)),
                          ("gt_ignore", gt_ignore, (Gt,)), ("dt_area", dt_area, (Dt,)), ("area_rng", area_rng, (A, 2))):
        _keval_shape(who, name, t, want)
    _ceval_limits(who, C=C, Gt=Gt, Dt=Dt, T=T, A=A)
    dtm = torch.empty((A, T, Dt), dtype=torch.int32, device=dev)
    dt_ig = torch.empty((A, T, Dt), dtype=torch.uint8, device=dev)
    cell_ngt = torch.empty((A, C), dtype=torch.int32, device=dev)
    _lib.call("md_coco_eval_match", [_i32c(gt_beg, dev), _i32c(gt_cnt, dev), _i32c(dt_beg, dev), _i32c(dt_cnt, dev), _f64c(gt_box, dev), _f64c(gt_area, dev),
                                     _u8c(gt_crowd, dev), _u8c(gt_ignore, dev), _f64c(dt_box, dev), _f64c(dt_area, dev), _f64c(iou_thr, dev),
                                     _f64c(area_rng, dev), dtm, dt_ig, cell_ngt])
    return dtm, dt_ig, cell_ngt


def coco_eval_accumulate(order, cat_off, dt_rank, dtm, dt_ig, cell_ngt, rec_thr, max_dets):
    """The body of COCOBboxEval.evaluate() (md_coco_eval_accumulate): order [Dt] i32 (detection rows, category-major, descending score,
    equal scores in row order), cat_off [Kc+1] i32, dt_rank [Dt] i32, coco_eval_match's three results, rec_thr [R] f64, max_dets [M] i32
    -> (precision [T,R,Kc,A,M] f64, recall [T,Kc,A,M] f64, n_gt [A,Kc] i32)."""
    who, dev = "coco_eval_accumulate", dtm.device
    if order.dim() != 1 or cat_off.dim() != 1 or cat_off.shape[0] < 2 or dtm.dim() != 3 or cell_ngt.dim() != 2 or rec_thr.dim() != 1 or max_dets.dim() != 1:
        raise ValueError(f"{who}: order is [Dt], cat_off [Kc + 1], dtm [A, T, Dt], cell_ngt [A, I Kc], rec_thr [R] and max_dets [M]")
    Dt, Kc, (A, T, _), C, R, M = order.shape[0], cat_off.shape[0] - 1, dtm.shape, cell_ngt.shape[1], rec_thr.shape[0], max_dets.shape[0]
    for name, t, want in (("dt_rank", dt_rank, (Dt,)), ("dtm", dtm, (A, T, Dt)), ("dt_ig", dt_ig, (A, T, Dt)), ("cell_ngt", cell_ngt, (A, C))):
        _keval_shape(who, name, t, want)
    if C < 1 or C % Kc:
        raise ValueError(f"{who}: {C} cells are no multiple of {Kc} categories")
    _ceval_limits(who, C=C, Kc=Kc, Dt=Dt, T=T, A=A, R=R, M=M)
    precision = torch.empty((T, R, Kc, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, Kc, A, M), dtype=torch.float64, device=dev)
    n_gt = torch.empty((A, Kc), dtype=torch.int32, device=dev)
    _lib.call("md_coco_eval_accumulate", [_i32c(order, dev), _i32c(cat_off, dev), _i32c(dt_rank, dev), _i32c(dtm, dev), _u8c(dt_ig, dev), _i32c(cell_ngt, dev),
                                          _f64c(rec_thr, dev), _i32c(max_dets, dev), precision, recall, n_gt])
    return precision, recall, n_gt


# ----------------------------------------------------------------------------- nuScenes detection evaluation (csrc/nusceval.hip)
NUSCEVAL_MAX_SAMPLE_DETS, NUSCEVAL_MAX_GTS, NUSCEVAL_MAX_CLASSES, NUSCEVAL_MAX_THRS = 512, 1024, 16, 8      # MD_NUSCEVAL_MAX_SAMPLE_DETS, _MAX_GTS, ...
NUSCEVAL_MAX_RECS, NUSCEVAL_MAX_CELLS, NUSCEVAL_MAX_ROWS, NUSCEVAL_MAX_LABELS = 256, 1 << 24, 1 << 26, 4096 # MD_NUSCEVAL_MAX_RECS, _MAX_CELLS, ...


class _NuscRowsAttrs(ctypes.Structure):
    _fields_ = [("first_sample", ctypes.c_int32)]


class _NuscEvalAttrs(ctypes.Structure):
    _fields_ = [("tp_index", ctypes.c_int32)]


def _neval_limits(who, C=1, Kc=1, Gt=0, Dt=0, D=1, R=1):
    if min(C, Kc, D, R) < 1:
        raise ValueError(f"{who}: at least one cell, class, distance threshold and recall point")
    if C >= NUSCEVAL_MAX_CELLS or Kc > NUSCEVAL_MAX_CLASSES or Gt > NUSCEVAL_MAX_ROWS or Dt > NUSCEVAL_MAX_ROWS:
        raise ValueError(f"{who}: fewer than {NUSCEVAL_MAX_CELLS} cells, at most {NUSCEVAL_MAX_CLASSES} classes and {NUSCEVAL_MAX_ROWS} rows, got "
                         f"{C}, {Kc}, {max(Gt, Dt)}")
    if D > NUSCEVAL_MAX_THRS or R > NUSCEVAL_MAX_RECS:
        raise ValueError(f"{who}: at most {NUSCEVAL_MAX_THRS} distance thresholds and {NUSCEVAL_MAX_RECS} recall points, got {D} and {R}")


def nusc_rows(dets, count, pose, label_to_k, class_range, attr_moving, attr_still, first_sample, dt_xyz, dt_size, dt_quat, dt_vel, dt_yaw, dt_score,
              dt_cat, dt_attr, dt_rank, dt_src, dt_beg, dt_cnt):
    """dets_to_nusc, the class-range filter and the grouping into (sample, class) cells for one batch, nothing read back (md_nusc_rows,
    include/minddet_hip_nusceval.h): dets [B,max_det,11] f32 (md_cp_pack's rows), count [B] i32, pose [B,14] f64 (cs_rotation,
    cs_translation, ego_rotation, ego_translation), label_to_k [L] i32 (-1 drops the row), class_range [Kc] f64, attr_moving, attr_still
    [Kc] i32.  The twelve outputs are the operands of the whole set (Dt = I max_det rows, I Kc cells), written in place for the samples
    first_sample .. first_sample + B - 1: dt_xyz, dt_size [Dt,3], dt_quat [Dt,4], dt_vel [Dt,2], dt_yaw, dt_score [Dt] f64, dt_cat,
    dt_attr, dt_rank, dt_src [Dt] i32, dt_beg, dt_cnt [I Kc] i32."""
    who = "nusc_rows"
    if dets.dim() != 3 or dets.shape[2] != 11 or dets.shape[1] < 1 or dets.dtype != torch.float32:
        raise ValueError(f"{who}: dets are [B, max_det, 11] float32, got {tuple(dets.shape)} {dets.dtype}")
    dev, (B, max_det) = dets.device, dets.shape[:2]
    if max_det > NUSCEVAL_MAX_SAMPLE_DETS:
        raise ValueError(f"{who}: at most {NUSCEVAL_MAX_SAMPLE_DETS} rows per sample, got {max_det}")
    if label_to_k.dim() != 1 or not 1 <= label_to_k.shape[0] <= NUSCEVAL_MAX_LABELS:
        raise ValueError(f"{who}: label_to_k is [L], 1 <= L <= {NUSCEVAL_MAX_LABELS}")
    if class_range.dim() != 1 or class_range.shape[0] < 1:
        raise ValueError(f"{who}: class_range is [Kc]")
    Kc = class_range.shape[0]
    for name, t, want in (("count", count, (B,)), ("pose", pose, (B, 14)), ("attr_moving", attr_moving, (Kc,)), ("attr_still", attr_still, (Kc,))):
        _keval_shape(who, name, t, want)
    if dt_xyz.dim() != 2 or dt_beg.dim() != 1 or dt_xyz.shape[0] < 1 or dt_xyz.shape[0] % max_det or dt_beg.shape[0] != dt_xyz.shape[0] // max_det * Kc:
        raise ValueError(f"{who}: dt_xyz is [I max_det, 3] and dt_beg [I Kc]")
    Dt, C = dt_xyz.shape[0], dt_beg.shape[0]
    I, f64, i32 = Dt // max_det, torch.float64, torch.int32
    outs = (("dt_xyz", dt_xyz, (Dt, 3), f64), ("dt_size", dt_size, (Dt, 3), f64), ("dt_quat", dt_quat, (Dt, 4), f64), ("dt_vel", dt_vel, (Dt, 2), f64),
            ("dt_yaw", dt_yaw, (Dt,), f64), ("dt_score", dt_score, (Dt,), f64), ("dt_cat", dt_cat, (Dt,), i32), ("dt_attr", dt_attr, (Dt,), i32),
            ("dt_rank", dt_rank, (Dt,), i32), ("dt_src", dt_src, (Dt,), i32), ("dt_beg", dt_beg, (C,), i32), ("dt_cnt", dt_cnt, (C,), i32))
    for name, t, want, dtype in outs:
        _keval_shape(who, name, t, want)
        if t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{who}: {name} is a contiguous {dtype} tensor on {dev} (it is written in place)")
    _neval_limits(who, C=C, Kc=Kc, Dt=Dt)
    if first_sample < 0 or first_sample + B > I:
        raise ValueError(f"{who}: samples {first_sample} .. {first_sample + B - 1} of {I}")
    _lib.call("md_nusc_rows", [dets.contiguous(), _i32c(count, dev), _f64c(pose, dev), _i32c(label_to_k, dev), _f64c(class_range, dev),
                               _i32c(attr_moving, dev), _i32c(attr_still, dev)] + [t for _, t, _, _ in outs], extra=_NuscRowsAttrs(int(first_sample)))


def nusc_eval_match(gt_beg, gt_cnt, dt_beg, dt_cnt, gt_xy, gt_size, gt_yaw, gt_vel, gt_attr, dt_xyz, dt_size, dt_yaw, dt_vel, dt_attr, dist_thr, period,
                    tp_index):
    """The greedy centre-distance matching of the devkit's accumulate() for every (sample, class) cell and all thresholds
    (md_nusc_eval_match): the cell tables [I Kc] i32, the ground-truth rows (gt_xy [Gt,2], gt_size [Gt,3], gt_yaw [Gt], gt_vel [Gt,2] f64,
    gt_attr [Gt] i32), the detection rows (dt_xyz [Dt,3], dt_size [Dt,3], dt_yaw [Dt], dt_vel [Dt,2] f64, dt_attr [Dt] i32), dist_thr [D]
    f64, period [Kc] f64, tp_index -> (dtm [D,Dt] i32: the packed ground-truth row matched or -1, err [Dt,5] f64: the five errors of the
    match at threshold tp_index, cell_ngt [I Kc] i32).  The per-cell counts are device data the kernel clamps; the packer refuses a cell
    beyond the limits."""
    who, dev = "nusc_eval_match", gt_xy.device
    if gt_beg.dim() != 1 or gt_xy.dim() != 2 or gt_xy.shape[1] != 2 or dt_xyz.dim() != 2 or dt_xyz.shape[1] != 3 or dist_thr.dim() != 1 or period.dim() != 1:
        raise ValueError(f"{who}: the cell tables are [I Kc], gt_xy [Gt, 2], dt_xyz [Dt, 3], dist_thr [D] and period [Kc]")
    C, Gt, Dt, D, Kc = gt_beg.shape[0], gt_xy.shape[0], dt_xyz.shape[0], dist_thr.shape[0], period.shape[0]
    for name, t, want in (("gt_cnt", gt_cnt, (C,)), ("dt_beg", dt_beg, (C,)), ("dt_cnt", dt_cnt, (C,)), ("gt_size", gt_size, (Gt, 3)), ("gt_yaw", gt_yaw, (Gt,)),
                          ("gt_vel", gt_vel, (Gt, 2)), ("gt_attr", gt_attr, (Gt,)), ("dt_size", dt_size, (Dt, 3)), ("dt_yaw", dt_yaw, (Dt,)),
                          ("dt_vel", dt_vel, (Dt, 2)), ("dt_attr", dt_attr, (Dt,))):
        _keval_shape(who, name, t, want)
    _neval_limits(who, C=C, Kc=Kc, Gt=Gt, Dt=Dt, D=D)
    if C % Kc or not 0 <= tp_index < D:
        raise ValueError(f"{who}: {C} cells are a multiple of {Kc} classes and tp_index lies in [0, {D}), got {tp_index}")
    dtm = torch.empty((D, Dt), dtype=torch.int32, device=dev)
    err = torch.empty((Dt, 5), dtype=torch.float64, device=dev)
    cell_ngt = torch.empty((C,), dtype=torch.int32, device=dev)
    _lib.call("md_nusc_eval_match", [_i32c(gt_beg, dev), _i32c(gt_cnt, dev), _i32c(dt_beg, dev), _i32c(dt_cnt, dev), _f64c(gt_xy, dev), _f64c(gt_size, dev),
                                     _f64c(gt_yaw, dev), _f64c(gt_vel, dev), _i32c(gt_attr, dev), _f64c(dt_xyz, dev), _f64c(dt_size, dev), _f64c(dt_yaw, dev),
                                     _f64c(dt_vel, dev), _i32c(dt_attr, dev), _f64c(dist_thr, dev), _f64c(period, dev), dtm, err, cell_ngt],
              extra=_NuscEvalAttrs(int(tp_index)))
    return dtm, err, cell_ngt


def nusc_eval_accumulate(order, cat_off, dt_score, dtm, err, cell_ngt, rec_thr, tp_index):
    """The curves of the devkit's accumulate() (md_nusc_eval_accumulate): order [Dt] i32 (detection rows, class-major, walking order
    across the samples), cat_off [Kc+1] i32, dt_score [Dt] f64, nusc_eval_match's three results, rec_thr [R] f64, tp_index ->
    (precision [Kc,D,R], confidence [Kc,D,R], tp_err [Kc,5,R] f64, n_gt [Kc], n_match [Kc,D] i32, tp_scan [D,Dt] i32, m_conf [Dt],
    m_cum [5,Dt] f64)."""
    who, dev = "nusc_eval_accumulate", dtm.device
    if order.dim() != 1 or cat_off.dim() != 1 or cat_off.shape[0] < 2 or dtm.dim() != 2 or cell_ngt.dim() != 1 or rec_thr.dim() != 1:
        raise ValueError(f"{who}: order is [Dt], cat_off [Kc + 1], dtm [D, Dt], cell_ngt [I Kc] and rec_thr [R]")
    Dt, Kc, D, C, R = order.shape[0], cat_off.shape[0] - 1, dtm.shape[0], cell_ngt.shape[0], rec_thr.shape[0]
    for name, t, want in (("dt_score", dt_score, (Dt,)), ("dtm", dtm, (D, Dt)), ("err", err, (Dt, 5))):
        _keval_shape(who, name, t, want)
    if C < 1 or C % Kc or not 0 <= tp_index < D:
        raise ValueError(f"{who}: {C} cells are a multiple of {Kc} classes and tp_index lies in [0, {D}), got {tp_index}")
    _neval_limits(who, C=C, Kc=Kc, Dt=Dt, D=D, R=R)
    f = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    i = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    outs = (f(Kc, D, R), f(Kc, D, R), f(Kc, 5, R), i(Kc), i(Kc, D), i(D, Dt), f(Dt), f(5, Dt))
    _lib.call("md_nusc_eval_accumulate", [_i32c(order, dev), _i32c(cat_off, dev), _f64c(dt_score, dev), _i32c(dtm, dev), _f64c(err, dev), _i32c(cell_ngt, dev),
                                          _f64c(rec_thr, dev)] + list(outs), extra=_NuscEvalAttrs(int(tp_index)))
    return outs


# ----------------------------------------------------------------------------- the training step behind the losses (csrc/convbwd.hip, optim.hip)
class _Conv1x1BwdAttrs(ctypes.Structure):
    """md_conv1x1_bwd_attrs (include/minddet_hip_train.h)"""
    _fields_ = [("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("x_c_off", ctypes.c_int32), ("dy_c_off", ctypes.c_int32),
                ("reserved0", ctypes.c_int32)]


class _AdamAttrs(ctypes.Structure):
    """md_adam_attrs (include/minddet_hip_train.h)"""
    _fields_ = [(n, ctypes.c_double) for n in ("lr", "beta1", "beta2", "beta1_power", "beta2_power", "eps", "weight_decay", "max_norm",
                                               "grad_scale", "reserved0")]


def conv1x1_bwd_weight_workspace_bytes(P, cin, cout):
    return _lib.workspace_bytes("md_conv1x1_bwd_weight", P, cin, cout)


def conv1x1_bwd_weight(x, dy, pc, x_c_off=0, dy_c_off=0, out=None, with_bias=True, workspace=True):
    """Weight and bias gradient of the pointwise layer `pc` (nn_ops.PackedConv of a 1x1 conv) on the device (md_conv1x1_bwd_weight):
    x [N,H,W,Cx] bf16, the layer's input at channels [x_c_off, x_c_off + pc.cin); dy [N,H,W,Cy] f32, d loss / d output at channels
    [dy_c_off, dy_c_off + pc.cout) (what a *_loss(grad=True) returns) -> (dw f32 of pc.w's shape, db f32 of pc.bias's shape or None),
    padding rows and columns +0.0.  out = (dw, db): written in place (views of a flat gradient buffer).  workspace=False: the
    library's scratch pool instead of a torch allocation."""
    who = "conv1x1_bwd_weight"
    if pc.kh != 1 or pc.kw != 1 or pc.stride != 1 or pc.pad != 0:
        raise ValueError(f"{who}: a 1x1 / stride 1 / pad 0 layer, got {pc.kh}x{pc.kw} stride {pc.stride} pad {pc.pad}")
    if x.dtype != torch.bfloat16 or x.dim() != 4 or dy.dtype != torch.float32 or dy.dim() != 4 or tuple(x.shape[:3]) != tuple(dy.shape[:3]):
        raise ValueError(f"{who}: x is [N,H,W,Cx] bfloat16 and dy [N,H,W,Cy] float32 over the same pixels, got {tuple(x.shape)} {x.dtype}, "
                         f"{tuple(dy.shape)} {dy.dtype}")
    rows, kpad = pc.w.shape
    if out is None:
        out = (torch.empty((rows, kpad), dtype=torch.float32, device=x.device),
               torch.empty((pc.bias.shape[0],), dtype=torch.float32, device=x.device) if with_bias else None)
    dw, db = out
    P = x.shape[0] * x.shape[1] * x.shape[2]
    ws = _lib.scratch("md_conv1x1_bwd_weight", (P, pc.cin, pc.cout), x.device) if workspace else None
    at = _Conv1x1BwdAttrs(int(pc.cin), int(pc.cout), int(x_c_off), int(dy_c_off), 0)
    _lib.call("md_conv1x1_bwd_weight", [x.contiguous(), dy.contiguous(), dw, db] + ([ws] if ws is not None else []), extra=at)
    return dw, db


class _ConvBwdBlock(ctypes.Structure):
    """md_conv_bwd_block (include/minddet_hip_convbwd.h)"""
    _fields_ = [("row0", ctypes.c_int32), ("rows", ctypes.c_int32), ("col0", ctypes.c_int32), ("cols", ctypes.c_int32)]


class _ConvBwdAttrs(ctypes.Structure):
    """md_conv_bwd_attrs (include/minddet_hip_convbwd.h)"""
    _fields_ = [("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("x_c_off", ctypes.c_int32), ("dy_c_off", ctypes.c_int32),
                ("kernel", ctypes.c_int32), ("korder", ctypes.c_int32), ("n_blocks", ctypes.c_int32), ("blocks", _ConvBwdBlock * 4),
                ("reserved0", ctypes.c_int32)]


class _Conv1x1BwdDataAttrs(ctypes.Structure):
    """md_conv1x1_bwd_data_attrs (include/minddet_hip_convbwd.h)"""
    _fields_ = [("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("dy_c_off", ctypes.c_int32), ("dx_c_off", ctypes.c_int32),
                ("act_c_off", ctypes.c_int32), ("reserved0", ctypes.c_int32)]


def conv_bwd_attrs(cin, cout, x_c_off=0, dy_c_off=0, kernel=1, korder=0, blocks=()):
    """md_conv_bwd_attrs; blocks: up to four (row0, rows, col0, cols)"""
    if len(blocks) > 4:
        raise ValueError(f"conv_bwd_weight: at most 4 blocks, got {len(blocks)}")
    at = _ConvBwdAttrs(int(cin), int(cout), int(x_c_off), int(dy_c_off), int(kernel), int(korder), len(blocks))
    for k, b in enumerate(blocks):
        at.blocks[k] = _ConvBwdBlock(*[int(v) for v in b])
    return at


def conv_bwd_weight_workspace_bytes(P, cin, cout, kernel):
    return _lib.workspace_bytes("md_conv_bwd_weight", P, cin, cout, kernel)


def conv_bwd_weight(x, dy, pc, x_c_off=0, dy_c_off=0, cout=None, blocks=(), out=None, with_bias=True, workspace=True):
    """Weight and bias gradient of the layer `pc` (nn_ops.PackedConv of a 1x1 or a 3x3 / stride 1 / pad 1 conv) on the device
    (md_conv_bwd_weight): x [N,H,W,Cx] bf16, the layer's input at channels [x_c_off, x_c_off + pc.cin); dy [N,H,W,Cy] f32, d loss / d
    output at channels [dy_c_off, dy_c_off + cout) (cout: pc.cout unless given) -> (dw f32 of pc.w's shape and K order, db f32 of
    pc.bias's shape or None), padding +0.0.  blocks: (row0, rows, col0, cols) ranges of (output, input) channels outside of which dw
    is +0.0 (a fused block-diagonal layer).  out = (dw, db): written in place.  workspace=False: the library's scratch pool."""
    who = "conv_bwd_weight"
    k = pc.kh
    if pc.kh != pc.kw or k not in (1, 3) or pc.stride != 1 or pc.pad != (k - 1) // 2:
        raise ValueError(f"{who}: a 1x1 or 3x3 / stride 1 / same-padding layer, got {pc.kh}x{pc.kw} stride {pc.stride} pad {pc.pad}")
    if x.dtype != torch.bfloat16 or x.dim() != 4 or dy.dtype != torch.float32 or dy.dim() != 4 or tuple(x.shape[:3]) != tuple(dy.shape[:3]):
        raise ValueError(f"{who}: x is [N,H,W,Cx] bfloat16 and dy [N,H,W,Cy] float32 over the same pixels, got {tuple(x.shape)} {x.dtype}, "
                         f"{tuple(dy.shape)} {dy.dtype}")
    rows, kpad = pc.w.shape
    cout = int(pc.cout if cout is None else cout)
    if out is None:
        out = (torch.empty((rows, kpad), dtype=torch.float32, device=x.device),
               torch.empty((pc.bias.shape[0],), dtype=torch.float32, device=x.device) if with_bias else None)
    dw, db = out
    P = x.shape[0] * x.shape[1] * x.shape[2]
    ws = _lib.scratch("md_conv_bwd_weight", (P, pc.cin, cout, k), x.device) if workspace else None
    at = conv_bwd_attrs(pc.cin, cout, x_c_off, dy_c_off, k, getattr(pc, "korder", 0) if k > 1 else 0, blocks)
    _lib.call("md_conv_bwd_weight", [x.contiguous(), dy.contiguous(), dw, db] + ([ws] if ws is not None else []), extra=at)
    return dw, db


def conv1x1_bwd_data(dy, pc, cin=None, cout=None, act=None, dy_c_off=0, dx_c_off=0, act_c_off=0, out=None):
    """Input gradient of the pointwise layer `pc` (md_conv1x1_bwd_data): dy [N,H,W,Cy] f32 at channels [dy_c_off, dy_c_off + cout), the
    layer's bf16 pack pc.w as the forward pass read it; act [N,H,W,Ca] bf16 = the layer's input where a ReLU made it (dx is +0.0 where
    act is not > 0) -> dx [N,H,W,Cdx] f32, written at channels [dx_c_off, dx_c_off + cin) (out: an existing tensor, its other
    channels are left alone; default a fresh [N,H,W,cin]).  cin / cout default to pc's."""
    who = "conv1x1_bwd_data"
    if pc.kh != 1 or pc.kw != 1 or pc.stride != 1 or pc.pad != 0:
        raise ValueError(f"{who}: a 1x1 / stride 1 / pad 0 layer, got {pc.kh}x{pc.kw} stride {pc.stride} pad {pc.pad}")
    if dy.dtype != torch.float32 or dy.dim() != 4 or (act is not None and (act.dtype != torch.bfloat16 or tuple(act.shape[:3]) != tuple(dy.shape[:3]))):
        raise ValueError(f"{who}: dy is [N,H,W,Cy] float32 and act [N,H,W,Ca] bfloat16 over the same pixels")
    cin, cout = int(pc.cin if cin is None else cin), int(pc.cout if cout is None else cout)
    if out is None:
        out = torch.empty(tuple(dy.shape[:3]) + (dx_c_off + cin,), dtype=torch.float32, device=dy.device)
    at = _Conv1x1BwdDataAttrs(cin, cout, int(dy_c_off), int(dx_c_off), int(act_c_off), 0)
    _lib.call("md_conv1x1_bwd_data", [dy.contiguous(), pc.w, None if act is None else act.contiguous(), out], extra=at)
    return out


def _grouped_bwd_check(who, pk, t, name, x_c_off):
    """the refusals both grouped gradients share: pk a nn_ops.PackedGrouped without a ReLU, t [N,H,W,C] holding every group's slice"""
    if getattr(pk, "relu", 0):
        raise ValueError(f"{who}: the gradient of a grouped conv with a ReLU behind it is not built")
    if x_c_off < 0 or x_c_off + 64 * pk.groups > t.shape[3]:
        raise ValueError(f"{who}: {pk.groups} groups of 64 channels from channel {x_c_off} do not fit {name} {tuple(t.shape)}")


def conv2d_grouped_bwd_data(dy, pk, act=None, x_c_off=0, out=None):
    """Input gradient of nn_ops.conv2d_grouped(x, pk, y, x_c_off) (md_conv2d_grouped_bwd_data, include/minddet_hip_groupedbwd.h): dy
    [N,H,W,Cy] f32 = d loss / d y in y's layout (pk.y_offs), the grouped pack pk.w as the forward pass read it; act [N,H,W,Ca] bf16 =
    the forward pass's x where a ReLU made it (dx is +0.0 where act is not > 0) -> dx [N,H,W,Cdx] f32, group g written at channels
    [x_c_off + 64 g, + 64) (out: an existing tensor, its other channels are left alone; default a fresh [N,H,W,x_c_off + 64 groups])."""
    who = "conv2d_grouped_bwd_data"
    if dy.dtype != torch.float32 or dy.dim() != 4 or (act is not None and (act.dtype != torch.bfloat16 or act.dim() != 4 or
                                                                          tuple(act.shape[:3]) != tuple(dy.shape[:3]))):
        raise ValueError(f"{who}: dy is [N,H,W,Cy] float32 and act [N,H,W,Ca] bfloat16 over the same pixels")
    if out is None:
        out = torch.empty(tuple(dy.shape[:3]) + (x_c_off + 64 * pk.groups,), dtype=torch.float32, device=dy.device)
    if out.dtype != torch.float32 or out.dim() != 4 or tuple(out.shape[:3]) != tuple(dy.shape[:3]):
        raise ValueError(f"{who}: out is [N,H,W,Cdx] float32 over dy's pixels, got {tuple(out.shape)} {out.dtype}")
    for t, name in ((out, "out"),) + (((act, "act"),) if act is not None else ()):
        _grouped_bwd_check(who, pk, t, name, x_c_off)
    _lib.call("md_conv2d_grouped_bwd_data", [dy.contiguous(), pk.w, None if act is None else act.contiguous(), out], extra=pk.attrs(x_c_off))
    return out


def conv2d_grouped_bwd_weight_workspace_bytes(P, groups, k):
    return _lib.workspace_bytes("md_conv2d_grouped_bwd_weight", P, groups, k)


def conv2d_grouped_bwd_weight(x, dy, pk, x_c_off=0, out=None, with_bias=True, workspace=True):
    """Weight and bias gradient of every group of nn_ops.conv2d_grouped(x, pk, y, x_c_off) in one pair of launches
    (md_conv2d_grouped_bwd_weight): x [N,H,W,C] bf16, dy [N,H,W,Cy] f32 = d loss / d y -> (dw f32 of pk.w's shape and layout, db f32 of
    pk.bias's shape or None); group g's rows are what conv_bwd_weight returns for that group alone, bit for bit.  out = (dw, db): written
    in place (views of a flat gradient buffer).  workspace=False: the library's scratch pool instead of a torch allocation."""
    who = "conv2d_grouped_bwd_weight"
    if x.dtype != torch.bfloat16 or x.dim() != 4 or dy.dtype != torch.float32 or dy.dim() != 4 or tuple(x.shape[:3]) != tuple(dy.shape[:3]):
        raise ValueError(f"{who}: x is [N,H,W,C] bfloat16 and dy [N,H,W,Cy] float32 over the same pixels, got {tuple(x.shape)} {x.dtype}, "
                         f"{tuple(dy.shape)} {dy.dtype}")
    _grouped_bwd_check(who, pk, x, "x", x_c_off)
    if out is None:
        out = (torch.empty(tuple(pk.w.shape), dtype=torch.float32, device=x.device),
               torch.empty((pk.w.shape[0],), dtype=torch.float32, device=x.device) if with_bias else None)
    dw, db = out
    P = x.shape[0] * x.shape[1] * x.shape[2]
    ws = _lib.scratch("md_conv2d_grouped_bwd_weight", (P, pk.groups, pk.k), x.device) if workspace else None
    _lib.call("md_conv2d_grouped_bwd_weight", [x.contiguous(), dy.contiguous(), dw, db] + ([ws] if ws is not None else []), extra=pk.attrs(x_c_off))
    return dw, db


def grad_sumsq_workspace_bytes(n):
    return _lib.workspace_bytes("md_grad_sumsq", n)


def grad_sumsq(grad, out=None, workspace=True):
    """sum of squares of a flat f32 gradient in float64, in a fixed order (md_grad_sumsq) -> [1] f64"""
    if grad.dtype != torch.float32 or grad.dim() != 1:
        raise ValueError(f"grad_sumsq: grad is a flat float32 tensor, got {tuple(grad.shape)} {grad.dtype}")
    if out is None:
        out = torch.empty((1,), dtype=torch.float64, device=grad.device)
    ws = _lib.scratch("md_grad_sumsq", (grad.shape[0],), grad.device) if workspace else None
    _lib.call("md_grad_sumsq", [grad, out] + ([ws] if ws is not None else []))
    return out


def adam_attrs(lr, beta1, beta2, beta1_power, beta2_power, eps=1e-8, weight_decay=0.0, max_norm=None, grad_scale=1.0):
    return _AdamAttrs(float(lr), float(beta1), float(beta2), float(beta1_power), float(beta2_power), float(eps), float(weight_decay),
                      0.0 if max_norm is None else float(max_norm), float(grad_scale), 0.0)


def adam_step(grad, param, m, v, *, lr, beta1, beta2, beta1_power, beta2_power, eps=1e-8, weight_decay=0.0, sumsq=None, max_norm=None,
              grad_scale=1.0, shadow=None):
    """One Adam.construct of the reference for a flat range, in place (md_adam_step, include/minddet_hip_train.h): grad, param, m, v
    [n] f32; sumsq [K] f64 with max_norm = the global-norm clip (None: none); beta1_power / beta2_power the running products, this step
    included; shadow [ns <= n] bf16 receives the new param[:ns]."""
    if (sumsq is None) != (max_norm is None):
        raise ValueError("adam_step: sumsq and max_norm come together (the global-norm clip) or not at all")
    at = adam_attrs(lr, beta1, beta2, beta1_power, beta2_power, eps, weight_decay, max_norm, grad_scale)
    _lib.call("md_adam_step", [grad, sumsq, param, m, v, shadow], extra=at)
    return param
