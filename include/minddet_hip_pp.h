/*
 * minddet_hip_pp.h -- C ABI of the anchor-based (KITTI) PointPillars head post-processing of libminddet_hip.so: the class scores of
 * every anchor in one pass, and the box decode of the selected anchors only.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions"), which this header includes.
 *
 * Both ops read the merged head tensor of the model in place: head[B,H,W,C] bf16 (NHWC) holds, per cell (y, x), the outputs of
 * conv_cls, conv_box and conv_dir_cls (minddet/models/pointpillars/src/pointpillars.py:562-578) side by side.  With A anchors per
 * cell the anchor index is n = (y * W + x) * A + a, N = H * W * A per sample -- the order of the reference's transpose to NHWC
 * followed by view(B, -1, K) / view(B, -1, 7) / view(B, -1, 2) (:604-610, :626-636).
 */
#ifndef MINDDET_HIP_PP_H_
#define MINDDET_HIP_PP_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_pp_head_attrs {
    int32_t off_cls;     /* first channel of conv_cls: anchor a, class k is channel off_cls + a * num_classes + k */
    int32_t off_box;     /* first channel of conv_box: anchor a, code j is channel off_box + a * 7 + j (md_pp_decode_selected) */
    int32_t off_dir;     /* first channel of conv_dir_cls: anchor a, bin d is channel off_dir + a * 2 + d; -1: no direction classifier */
    int32_t num_anchors; /* A, anchors per cell */
    int32_t num_classes; /* K (md_pp_scores) */
    int32_t score_mode;  /* md_pp_scores: 0 = encode_background_as_zeros with sigmoid scores; anything else is not built (2) */
    int32_t self_train;  /* md_pp_decode_selected: 1 = the +pi direction fix below; 0 (the limit_period form, :637-649) is not built (2) */
} md_pp_head_attrs;

/* get_total_scores + get_selected_data up to the mask (pointpillars.py:741-763), for B samples in one launch.
 * in : head[B,H,W,C] bf16, mask[B,N] u8 or NULL (all valid)
 * out: scores[B,N] f32, labels[B,N] i32
 * extra: md_pp_head_attrs, required (off_cls, num_anchors, num_classes, score_mode are read).
 * Per anchor, in fp32: s_k = 1.0f / (1.0f + expf(-x_k)) of the K bf16 logits; score = the maximum of the s_k, label = the first k
 * that attains it (ops.max; 0 for K = 1); score = -1 where mask == 0 (the label is written all the same).
 * 2: num_anchors or num_classes <= 0, off_cls < 0 or off_cls + A K > C, score_mode != 0, output or mask shapes other than [B,N].
 * 4: B N or B H W C >= 2^31. */
int md_pp_scores(MD_AOT_ARGS);

/* generate_predicted_boxes (pointpillars.py:623-652) on the selected anchors only, then the direction fix of
 * pointpillars/src/predict.py:222-236 and the NMS operand of predict.py:61-78.
 * in : head[B,H,W,C] bf16, anchors[N,7] f32 (x, y, z, w, l, h, r), idx[B,k] i32 (anchor index per selected row), cnt[B] i32 (valid
 *      leading rows, clamped to k), sel_scores[B,k] f32 (the top-k's values), labels[B,N] i32 (md_pp_scores' output)
 * out: dets[B,k,9] f32 = (x, y, z, w, l, h, rot, score, label), standup[B,k,4] f32 (xmin, ymin, xmax, ymax), dir_labels[B,k] i32
 *      [, boxes[B,k,7] f32 or NULL: the decoded box before the direction fix]
 * extra: md_pp_head_attrs, required (off_box, off_dir, num_anchors, self_train are read).
 * Per row j < cnt[b] with n = idx[b,j]: the box is second_box_decode (pointpillars/src/core/box_ops.py:47-85, the non-vector angle
 * form) of the 7 bf16 encodings of anchor n widened to fp32 -- the same device function as md_second_box_decode, so the two agree bit
 * for bit; standup is the standup box of (x, y, w, l, rot) BEFORE the direction fix -- the same device function as md_standup_boxes;
 * dir_label = 1 if the second direction logit is greater than the first, else 0 (argmax, the first on a tie; 0 without a direction
 * classifier); with a direction classifier rot += (float)M_PI where (rot > 0) != (dir_label != 0); score = sel_scores[b,j]; label =
 * (float)labels[b,n].  Rows j >= cnt[b] are all zero.  idx lives on the device, so it cannot be checked here: a row whose n is outside
 * [0, N) is written as zeros too and nothing is read for it.
 * 2: num_anchors <= 0, off_box < 0 or off_box + 7 A > C, off_dir < -1 or off_dir + 2 A > C, self_train != 1, anchors rows != N,
 *    k or B not the same in idx, sel_scores and the outputs, labels not [B,N].
 * 4: B N, B k x 9 or B H W C >= 2^31. */
int md_pp_decode_selected(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_PP_H_ */
