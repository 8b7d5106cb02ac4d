"""One valid small call per MD_AOT_ARGS entry point of libminddet_hip.so, written from include/minddet_hip.h: operand shapes, dtypes,
the attribute struct, and which operands are optional.  tests/test_abi_checks_cpu.py derives single-defect calls from each row (tests/abi_derive.py,
as each feature's CPU test file does from its tests/abi_cases_*.py table; no GPU: the argument checks complete before any device call);
tests/test_abi_accept_gpu.py makes each row once with zero-filled tensors and expects rc 0, which is what proves the derived calls
carry ONE defect.  Zero indices, counts and offsets are in range for every row.

Operand kinds
  req    required: described (ndims[i], shapes[i]), dtype as documented, data pointer non-NULL when the call has work
  opt    "or NULL" in the header: a NULL pointer passes with nothing else looked at; null=True passes NULL in the valid row
  loose  thresh / outputs of the five reference-ABI ops: the caller may leave shapes[i] NULL (nms.hip: "shapes a caller does not
         describe are not checked"), so neither a NULL shapes[i] nor a rank defect applies; dtype and data pointer still do
rank: what a rank +- 1 defect (append an extent of 2 / drop the last extent) must give
  exact  both are rc 2 (the op pins the rank or the element count)
  min    the op needs AT LEAST the documented elements: only the shrinking defect (rank - 1) is rc 2
  free   neither applies; `why` says why
"""
import ctypes as C

i32, f32, f64 = C.c_int32, C.c_float, C.c_double


def S(*fields):
    """ctypes mirror of a header struct: S(("name", type), ...)"""
    return type("Attrs", (C.Structure,), {"_fields_": list(fields)})


class T:
    def __init__(self, shape, dtype, kind="req", rank="exact", null=False, why=None):
        assert kind in ("req", "opt", "loose") and rank in ("exact", "min", "free")
        assert rank != "free" or why or kind != "req", "a free-rank required operand says why"
        self.shape, self.dtype, self.kind, self.rank, self.null, self.why = tuple(shape), dtype, kind, rank, null, why


class Case:
    def __init__(self, sym, operands, extra=None, extra_required=False, nparam=None, tag=""):
        self.sym, self.operands, self.extra, self.extra_required, self.tag = sym, operands, extra, extra_required, tag
        self.nparam = set(nparam) if nparam else {len(operands)}     # the allowed parameter counts (a trailing workspace is optional)

    @property
    def id(self):
        return self.sym + self.tag


F, B16, I, I64, U8 = "float32", "bfloat16", "int32", "int64", "uint8"
FLT_MAX = 3.4028234663852886e38

Delta = S(("means", f32 * 4), ("stds", f32 * 4), ("max_ratio", f32), ("clip_w", f32), ("clip_h", f32))
ConvTune = S(*[(n, i32) for n in ("chunk_limit", "stream_rounds", "stream_wgs_per_cu", "stream_cache_bits", "pers_min_k", "dual_pp_min_k")])
Conv2d = S(*[(n, i32) for n in ("kh", "kw", "stride", "pad", "relu", "variant", "adv", "pad_top", "pad_left", "sub_h", "sub_w", "out_stride",
                                 "out_off_y", "out_off_x", "c_off", "cout", "res_upsample", "korder", "x_c_off", "x_cin", "res_slice", "res_c_off",
                                 "reserved0")], ("tune", ConvTune))
Grouped = S(("k", i32), ("relu", i32), ("groups", i32), ("cin_g", i32), ("x_c_off", i32), ("reserved0", i32), ("cout", i32 * 64),
            ("y_off", i32 * 64), ("w_row", i32 * 64))
Pool = S(("k", i32), ("stride", i32), ("pad", i32), ("zero_pad", i32))
Slice = S(("c0", i32), ("width", i32))


def _delta():
    return Delta((f32 * 4)(0, 0, 0, 0), (f32 * 4)(1, 1, 1, 1), 4.135, 0.0, 0.0)


def _keep_nms(sym, keep_dtype):
    why = "reference ABI: undescribed shapes are not checked"
    return Case(sym, [T((4, 7), F), T((1,), F, "loose", "free", why=why), T((4,), keep_dtype, "loose", "free", why=why),
                      T((1,), I, "loose", "free", why=why)], nparam={4, 5})


def _rot_matrix(sym):
    return Case(sym, [T((2, 7), F), T((3, 7), F), T((2, 3), F, "loose", "free", why="reference ABI: undescribed shapes are not checked")],
                nparam={3, 4})


def _cases():
    c = []
    c += [_rot_matrix("BoxesIouBevGpu"), _rot_matrix("BoxesOverlapBevGpu"), _keep_nms("NmsGpu", I64), _keep_nms("NmsNormalGpu", I64),
          _keep_nms("boxes_iou_nms_gpu", I)]
    c.append(Case("md_iou_aligned", [T((2, 4), F), T((3, 4), F), T((2, 3), F, rank="min")], extra=S(("eps", f32))(0.0)))
    c.append(Case("md_rotate_iou_eval", [T((2, 5), F), T((3, 5), F), T((2, 3), F, rank="min")], extra=S(("criterion", i32))(-1)))
    one = "one element: dropping its extent leaves a scalar, still one element"
    # (the [N,4] form: a [B,N,4] row minus its last extent would be a valid [N,4] call)
    c.append(Case("md_nms_aligned", [T((4, 4), F), T((1,), I, "opt", "free"), T((4,), I, "opt", "min"), T((4,), U8, rank="min"), T((4,), I, rank="min"),
                                     T((1,), I, rank="free", why=one)],
                  extra=S(("iou_threshold", f32), ("eps", f32), ("mode", i32), ("max_output", i32))(0.5, 0.0, 0, 0), extra_required=True, nparam={6, 7}))
    c.append(Case("md_soft_nms", [T((2, 4, 4), F), T((2, 4), F), T((2,), I, "opt", "min"), T((2, 4), F), T((2, 4), I), T((2,), I)],
                  extra=S(("sigma", f32), ("Nt", f32), ("threshold", f32), ("method", i32))(0.5, 0.5, 0.001, 1), extra_required=True))
    c.append(Case("md_circle_nms", [T((4, 2), F), T((1,), F, rank="free", why=one), T((4,), U8, rank="min"), T((4,), I, rank="min"),
                                    T((1,), I, rank="free", why=one)], nparam={5, 6}))
    # conv family
    c.append(Case("md_conv2d", [T((1, 8, 8, 64), B16), T((64, 64), B16), T((64,), F), T((1, 8, 8, 64), B16, "opt"), T((1, 8, 8, 64), B16)],
                  extra=Conv2d(1, 1, 1, 0, 0), extra_required=True))
    c.append(Case("md_conv1x1_dual", [T((1, 8, 8, 64), B16), T((1, 8, 8, 64), B16), T((128, 128), B16), T((128,), F), T((1, 8, 8, 128), B16, "opt"),
                                      T((1, 8, 8, 128), B16)],
                  extra=S(("stride_b", i32), ("relu", i32), ("tune", ConvTune))(1, 0), extra_required=True))
    c.append(Case("md_conv2d_head", [T((1, 16, 16, 64), B16), T((256, 576), B16), T((256,), F), T((32, 256), B16), T((32,), F, rank="min"),
                                     T((1, 16, 16, 16), B16)], extra=Conv2d(3, 3, 1, 1, 1), extra_required=True, nparam={6, 7}))
    c.append(Case("md_bottleneck", [T((1, 8, 8, 256), B16), T((64, 256), B16), T((128,), F), T((64, 576), B16), T((256, 64), B16),
                                    T((256,), F, rank="min"), T((1, 8, 8, 256), B16, "opt", null=True), T((256, 64), B16, "opt", null=True),
                                    T((256,), F, "opt", null=True), T((1, 8, 8, 256), B16)]))
    c.append(Case("md_c3_pair", [T((1, 8, 8, 64), B16), T((64, 64), B16), T((128,), F), T((64, 576), B16), T((1, 8, 8, 64), B16)],
                  extra=S(("x_c_off", i32), ("y_c_off", i32), ("shortcut", i32), ("pass_through", i32))(0, 0, 1, 0), extra_required=True))
    g = Grouped(3, 0, 1, 64, 0, 0)
    g.cout[0] = 2
    c.append(Case("md_conv2d_grouped", [T((1, 8, 8, 64), B16), T((2, 576), B16), T((2,), F), T((1, 8, 8, 8), B16)], extra=g, extra_required=True))
    # streaming helpers
    c.append(Case("md_maxpool2d", [T((1, 8, 8, 8), B16), T((1, 4, 4, 8), B16)], extra=Pool(2, 2, 0, 0), extra_required=True))
    c.append(Case("md_sppf_pool", [T((1, 8, 8, 32), B16)], extra=S(("channels", i32), ("k", i32))(8, 5), extra_required=True))
    c.append(Case("md_yolov8_decode", [T((1, 4, 4, 72), B16), T((1, 16, 4), F), T((1, 16), F), T((1, 16), I)],
                  extra=S(("num_classes", i32), ("reg_max", i32), ("stride", f32), ("conf_thres", f32), ("out_offset", i32),
                          ("out_total", i32))(8, 16, 8.0, 0.25, 0, 16), extra_required=True))
    c.append(Case("md_mask_select", [T((2, 4, 4, 8), B16), T((2, 6), F), T((2, 4, 4), F)], extra=i32(3), extra_required=True))
    c.append(Case("md_paste_masks", [T((2, 4, 4), F), T((2, 6), F), T((2, 16, 1), I)],
                  extra=S(("img_h", i32), ("img_w", i32), ("threshold", f32), ("bits", i32))(16, 16, 0.5, 1), extra_required=True))
    c.append(Case("md_assign_targets", [T((4, 7), F), T((2, 7), F, "opt"), T((2,), I, "opt"), T((4,), F), T((4,), F), T((4,), U8, "opt"), T((4,), I),
                                        T((4, 7), F), T((4,), F), T((4,), I)], nparam={10, 11}))
    c.append(Case("md_image_preprocess", [T((1, 8, 8, 3), U8), T((1, 6), F), T((6,), F), T((1, 8, 8, 8), B16)],
                  extra=S(("out_h", i32), ("out_w", i32), ("pad_lo", i32), ("pad_hi", i32))(8, 8, 0, 0), extra_required=True))
    c.append(Case("md_deform_cols", [T((1, 8, 8, 8), B16), T((1, 8, 8, 32), B16), T((1, 8, 8, 72), B16)], extra=Pool(3, 1, 1, 0), extra_required=True))
    c.append(Case("md_stem_pool", [T((1, 32, 80, 4), B16), T((64, 224), B16), T((64,), F), T((1, 4, 16, 64), B16)]))
    c.append(Case("md_stem_conv", [T((1, 32, 80, 4), B16), T((32, 192), B16), T((32,), F), T((1, 8, 32, 32), B16)],
                  extra=S(("kh", i32), ("act", i32))(6, 2), extra_required=True))
    c.append(Case("md_upsample_add", [T((1, 8, 8, 8), B16), T((1, 4, 4, 8), B16), T((1, 8, 8, 8), B16)]))
    c.append(Case("md_slice_cast", [T((2, 4, 8), B16), T((2, 4, 4), F)], extra=Slice(0, 4), extra_required=True))
    c.append(Case("md_concat_copy", [T((1, 4, 4, 8), B16), T((1, 4, 4, 16), B16)], extra=Slice(8, 8), extra_required=True))
    c.append(Case("md_upsample2x", [T((1, 4, 4, 8), B16), T((1, 8, 8, 16), B16)], extra=S(("c0", i32), ("width", i32), ("src_c0", i32))(8, 8, 0),
                  extra_required=True))
    c.append(Case("md_nhwc_to_nchw_f32", [T((1, 4, 4, 8), B16), T((1, 4, 4, 4), F)], extra=Slice(0, 4), extra_required=True))
    # anchors
    fpn = S(("num_levels", i32), ("num_ratios", i32), ("feat_h", i32 * 8), ("feat_w", i32 * 8), ("stride", i32 * 8), ("scale", f32),
            ("ratios", f32 * 16))(1, 3)
    fpn.feat_h[0], fpn.feat_w[0], fpn.stride[0], fpn.scale = 4, 4, 8, 8.0
    fpn.ratios[0], fpn.ratios[1], fpn.ratios[2] = 0.5, 1.0, 2.0
    c.append(Case("md_anchors_fpn", [T((48, 4), F)], extra=fpn, extra_required=True))
    a3 = S(("feat_h", i32), ("feat_w", i32), ("num_rot", i32), ("range", f64 * 6), ("z_offset", f64), ("size", f64 * 3), ("rotations", f64 * 8),
           ("slot_off", i32), ("slots_total", i32))(2, 2, 2, (f64 * 6)(0, -40, -3, 70, 40, 1), -1.78, (f64 * 3)(1.6, 3.9, 1.56), (f64 * 8)(0, 1.57), 0, 0)
    c.append(Case("md_anchors_3d_stride", [T((1, 2, 2, 1, 2, 7), F)], extra=a3, extra_required=True))
    a3r = S(("feat_d", i32), ("feat_h", i32), ("feat_w", i32), ("num_sizes", i32), ("num_rot", i32), ("linspace_mode", i32), ("slot_off", i32),
            ("slots_total", i32), ("range", f64 * 6), ("sizes", (f64 * 3) * 4), ("rotations", f64 * 8))(1, 2, 2, 1, 2, 0, 0, 0)
    for k, v in enumerate((0, -40, -1.78, 70, 40, -1.78)):
        a3r.range[k] = v
    for k, v in enumerate((1.6, 3.9, 1.56)):
        a3r.sizes[0][k] = v
    a3r.rotations[1] = 1.57
    c.append(Case("md_anchors_3d_range", [T((1, 2, 2, 1, 2, 7), F)], extra=a3r, extra_required=True))
    c.append(Case("md_anchor_mask", [T((3, 3), I), T((4, 4), F), T((4,), F, rank="min"), T((4,), U8, rank="min")],
                  extra=S(("grid_x", i32), ("grid_y", i32), ("voxel_x", f32), ("voxel_y", f32), ("offset_x", f32), ("offset_y", f32),
                          ("area_threshold", f32))(8, 8, 0.16, 0.16, 0.0, 0.0, 1.0), extra_required=True, nparam={4, 5}))
    # codecs, top-k, RoIAlign
    c.append(Case("md_second_box_decode", [T((4, 7), F), T((4, 7), F), T((4, 7), F)]))
    c.append(Case("md_delta2bbox", [T((4, 4), F), T((4, 4), F), T((4, 4), F)], extra=_delta(), extra_required=True))
    c.append(Case("md_topk_segmented", [T((8,), F, rank="free", why="T is not known to the host: seg_off lives on the device"), T((3,), I), T((2, 2), F),
                                        T((2, 2), I), T((2,), I)],
                  extra=S(("k", i32), ("min_score", f32), ("max_segment", i32))(2, -FLT_MAX, 0), extra_required=True, nparam={5, 6}))
    roi = S(("num_levels", i32), ("pooled", i32), ("sampling_ratio", i32), ("aligned", i32), ("k_min", i32), ("canonical_level", i32),
            ("canonical_scale", f32), ("spatial_scale", f32 * 6))(2, 2, 2, 1, 2, 4, 224.0, (f32 * 6)(0.25, 0.125))
    c.append(Case("md_roi_align", [T((2, 5), F), T((1, 8, 8, 8), B16), T((1, 4, 4, 8), B16), T((2, 2, 2, 8), B16), T((2,), I, "opt", "min")], extra=roi,
                  extra_required=True))
    # CenterNet decode
    c.append(Case("md_sigmoid_clip", [T((2, 4), F), T((2, 4), F)], extra=S(("lo", f32), ("hi", f32))(1e-4, 1 - 1e-4)))
    c.append(Case("md_heat_nms", [T((1, 2, 4, 4), F), T((1, 2, 4, 4), F)]))
    c.append(Case("md_heat_peaks", [T((1, 4, 4, 8), B16), T((1, 2, 4, 4), F), T((1, 2, 4, 4), F, "opt")],
                  extra=S(("c0", i32), ("num_classes", i32), ("lo", f32), ("hi", f32))(0, 2, 1e-4, 1 - 1e-4), extra_required=True))
    c.append(Case("md_centernet_assemble", [T((2, 3), F), T((2, 3), I, rank="min"), T((2, 2, 3), I), T((2, 2, 4, 4), F), T((2, 2, 4, 4), F, "opt", "min"),
                                            T((2, 3, 6), F), T((2, 3), I, rank="min"), T((2, 3), I, rank="min")]))
    # two-stage glue
    c.append(Case("md_rpn_decode", [T((2, 4, 4, 8), B16), T((16, 4), F), T((2, 3), I), T((2,), I, rank="min"), T((2, 3, 4), F), T((2, 3), F)],
                  extra=S(("num_anchors", i32), ("decode", Delta))(1, _delta()), extra_required=True))
    c.append(Case("md_rpn_merge", [T((2, 2, 3, 4), F), T((2, 2, 3), F), T((2, 2, 3), U8), T((2, 6, 4), F), T((2, 6), F)]))
    c.append(Case("md_make_rois", [T((2, 6, 4), F), T((2, 3), F), T((2, 3), I, rank="min"), T((2,), I, rank="min"), T((6, 5), F), T((6,), F)]))
    Rcnn = S(("num_classes", i32), ("reg_offset", i32), ("score_thr", f32), ("decode", Delta))
    c.append(Case("md_rcnn_scores", [T((4, 16), B16), T((2,), I, rank="free", why="its element count IS the batch size B (any B dividing R)"),
                                     T((2, 6), F)], extra=Rcnn(3, 4, 0.05, _delta()), extra_required=True))
    c.append(Case("md_rcnn_decode_selected", [T((4, 16), B16), T((4, 5), F, rank="min"), T((2, 3), I), T((2,), I, rank="min"), T((2, 3, 4), F),
                                              T((2, 3), I)], extra=Rcnn(3, 4, 0.0, _delta()), extra_required=True))
    pack = [T((2, 3, 4), F, rank="min"), T((2, 3), F), T((2, 3), I, rank="min"), T((2, 3), I, rank="min"), T((2,), I, rank="min")]
    c.append(Case("md_pack_detections", pack + [T((2, 5, 6), F), T((2,), I, rank="min")], nparam={7, 9}))
    c.append(Case("md_pack_detections", pack + [T((2,), I), T((2, 5, 6), F), T((2,), I, rank="min"), T((2,), I)], nparam={7, 9}, tag="[status]"))
    # CenterPoint, misc, YOLOv5
    cp = S(("off_reg", i32), ("off_height", i32), ("off_dim", i32), ("off_rot", i32), ("off_vel", i32), ("off_hm", i32), ("num_classes", i32),
           ("score_threshold", f32), ("out_size_factor", f32), ("voxel_size", f32 * 2), ("pc_range", f32 * 2),
           ("post_center_range", f32 * 6))(0, 2, 3, 6, -1, 8, 2, 0.1, 4.0, (f32 * 2)(0.2, 0.2), (f32 * 2)(-51.2, -51.2),
                                           (f32 * 6)(-61.2, -61.2, -10, 61.2, 61.2, 10))
    c.append(Case("md_centerpoint_decode", [T((1, 4, 4, 16), B16), T((1, 16), F), T((1, 16), I), T((1, 16, 9), F), T((1, 16, 7), F)], extra=cp,
                  extra_required=True))
    c.append(Case("md_gather_rows", [T((2, 4, 3), F), T((2, 2), I), T((2,), I, "opt", "min"), T((2, 2, 3), F)]))
    c.append(Case("md_standup_boxes", [T((4, 5), F), T((4, 4), F)]))
    c.append(Case("md_yolo_decode", [T((1, 4, 4, 24), B16), T((1, 48, 4), F), T((1, 48), F), T((1, 48), I)],
                  extra=S(("num_classes", i32), ("num_anchors", i32), ("stride", f32), ("anchors", f32 * 6), ("conf_thres", f32), ("out_offset", i32),
                          ("out_total", i32))(3, 3, 8.0, (f32 * 6)(10, 13, 16, 30, 33, 23), 0.25, 0, 48), extra_required=True))
    return c


CASES = _cases()
