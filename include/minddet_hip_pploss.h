/*
 * minddet_hip_pploss.h -- C ABI of the KITTI PointPillars training loss of libminddet_hip.so: PointPillarsWithLossCell.construct behind
 * the network (minddet/models/pointpillars/src/pointpillars.py:817-872) with prepare_loss_weights (:19-43), create_loss (:64-98),
 * add_sin_difference (:101-107), _get_pos_neg_loss (:110-127), get_direction_target (:142-164, the use_self_train=True form) and the
 * three loss classes of minddet/models/pointpillars/src/core/losses.py:40-191, for a whole batch, on the merged head tensor of
 * md_pp_scores (minddet_hip_pp.h) and the labels / bbox_targets of md_assign_targets (minddet_hip.h).  Three launches, no host read,
 * no memset, no atomics on floating-point values: the result is the same from call to call and from stream to stream.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 */
#ifndef MINDDET_HIP_PPLOSS_H_
#define MINDDET_HIP_PPLOSS_H_

#include "minddet_hip_pp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_PP_LOSS_MAX_CHANNELS 128  /* C: a strip of 64 cells of head and grad, and its 64 A labels, are staged in LDS (A <= C / 8) */
#define MD_PP_LOSS_STRIP 64          /* cells per workgroup of the dense pass (the workspace formula) */
#define MD_PP_LOSS_COUNT_CHUNK 4096  /* labels per workgroup of the positive count (the workspace formula) */

typedef struct md_pp_loss_attrs {
    md_pp_head_attrs head;     /* off_cls, off_box, off_dir (-1: no direction loss), num_anchors, num_classes are read;
                                  score_mode != 0 or self_train != 1 -> 2 */
    float alpha;               /* focal alpha; < 0 = None (no alpha factor) */
    float gamma;               /* focal gamma >= 0; 0 = no modulating factor (losses.py:87-89) */
    float sigma;               /* smooth-L1 sigma > 0 */
    float code_weights[7];
    float cls_weight, loc_weight, dir_weight;   /* classification_weight, localization_weight, direction_loss_weight */
    float pos_cls_weight, neg_cls_weight;       /* both > 0: the two diagnostics are divided by them */
} md_pp_loss_attrs;

/* PointPillarsWithLossCell.construct (pointpillars.py:817-872) behind the network, for a batch.
 * in : head[B,H,W,C] bf16 (raw outputs of conv_cls, conv_box, conv_dir_cls at the channels `head` names; any channel no head owns is
 *      padding: its value never enters the arithmetic), labels[B,N] i32 (-1 ignore, 0 background, k >= 1 a class), reg_targets[B,N,7]
 *      f32, anchors[N,7] f32 ; N = H W A, anchor n = (y W + x) A + a
 * out: parts[5] f32 = (loc, cls, dir as they enter the total, cls_pos, cls_neg), num_pos[B] f32, total[1] f32 ;
 *      md_pp_loss_grad only: grad[B,H,W,C] f32 = d total / d head, every element written (zeros and padding channels included) ;
 *      [workspace u8, 8-byte aligned: md_pp_loss_workspace_bytes(B, H, W, A) bytes (one function for both entry points), at least
 *      40 B ceil(H W / MD_PP_LOSS_STRIP) + 4 B ceil(N / MD_PP_LOSS_COUNT_CHUNK); without it the library's per-stream scratch pool
 *      serves]
 * extra: md_pp_loss_attrs, required.  B, H, W >= 1.  K = num_classes, A = num_anchors.
 *
 * As real-valued math on the given bf16 and fp32 values.  Arithmetic: every per-element term and every sum is evaluated in float64
 * and rounded once to fp32 on output (a choice: the reference's MindSpore fp32 kernels are not pinned by its source, and the literal
 * fp32 1 - p is exactly 0 beyond |x| ~ 17).  Per sample b:
 *   pos, neg    labels > 0, labels == 0 ; n_b = max(number of positives, 1), the exact count, for all three normalisers
 *               (prepare_loss_weights :30-42 and construct :826-833; the reference sums the positives in float16, exact up to 2048).
 *               num_pos[b] = the number of positives.
 *   cls term    per anchor and class k < K: z = 1 if labels == k + 1 else 0 (a label above K is a positive whose row is all zero, as
 *               OneHot gives), w = (pos pos_cls_weight + neg neg_cls_weight) / n_b (0 on an ignored anchor), s = -x where z = 1 and
 *               x elsewhere, ce = max(s, 0) + log1p(exp(-|s|)), m = sigmoid(s) (this is 1 - p_t; never formed as 1 - sigmoid),
 *               alpha_t = alpha where z = 1 else 1 - alpha (1 with alpha < 0); term = m^gamma alpha_t ce w (losses.py:40-99, with
 *               clip(logits, 0, logits.max()) taken as max(x, 0)).
 *   loc term    positives only; every other anchor contributes exactly 0 and its targets are never read.  d_j = cw_j (pred_j - tgt_j)
 *               for j < 6, d_6 = cw_6 (sin pred_6 cos tgt_6 - cos pred_6 sin tgt_6) (add_sin_difference); term = 0.5 (sigma d)^2 if
 *               |d| <= 1 / sigma^2 else |d| - 0.5 / sigma^2, divided by n_b (losses.py:102-154, codewise).
 *   dir term    positives only, and only with off_dir >= 0: target bin t = 1 if the fp32 sum reg_targets[.., 6] + anchors[.., 6] is
 *               > 0 else 0 (get_direction_target); term = softplus(x_other - x_t) / n_b (the softmax cross-entropy of two logits).
 *   loc = loc_weight sum / B, cls = cls_weight sum / B, dir = dir_weight sum / B (0 without a direction head), total = loc + cls + dir.
 *   cls_pos, cls_neg  _get_pos_neg_loss literally: K = 1: the positives' and the negatives' cls terms, K > 1: the columns k >= 1 and
 *               column 0; summed, divided by B and by pos_cls_weight / neg_cls_weight (cls_weight does not enter).
 *   grad        the exact derivative of total.  cls channels: +-(cls_weight / B) alpha_t w m^gamma (gamma (1 - m) ce + m), - where
 *               z = 1.  box channels: (loc_weight / B) cw_j (sigma^2 d if |d| <= 1 / sigma^2 else sign d) / n_b, for j = 6 times
 *               cos(pred_6 - tgt_6).  dir channels: +-(dir_weight / B) sigmoid(x_other - x_t) / n_b, - on the target bin.  Exactly
 *               +0.0 on padding channels, on the cls channels of ignored anchors and on the box / dir channels of non-positive anchors.
 * md_pp_loss and md_pp_loss_grad give bit-identical parts, num_pos and total.
 * 2: an extent other than documented, B, H or W < 1, num_anchors or num_classes < 1, a head's channels not inside [0, C) or two heads
 *    sharing a channel, off_dir < -1, score_mode != 0, self_train != 1, gamma < 0, sigma <= 0, a non-finite attribute, pos_cls_weight
 *    or neg_cls_weight <= 0, a workspace that is not 8-byte aligned.
 * 4: C > MD_PP_LOSS_MAX_CHANNELS (so A <= 16: conv_cls and conv_box need 8 A channels), an operand of 2^30 elements or more,
 *    B > 65535, a workspace smaller than documented. */
int md_pp_loss(MD_AOT_ARGS);      /* forward only */
int md_pp_loss_grad(MD_AOT_ARGS); /* forward + d total / d head, in the same passes */
int64_t md_pp_loss_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t num_anchors);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_PPLOSS_H_ */
