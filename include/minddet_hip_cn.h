/*
 * minddet_hip_cn.h -- C ABI of the CenterNet training tail of libminddet_hip.so: the target part of COCOHP.preprocess_fn
 * (minddet/models/centernet/src/dataset.py:317-384 with gaussian_radius / gaussian2D / draw_umich_gaussian, src/image.py:94-144) and
 * CenterNetLossCell.construct behind the network (src/centernet_det.py:177-237 with FocalLoss and RegLoss, src/utils.py:48-245), each
 * for a batch, on the head tensor of graphs.CenterNet.features.  No host read, no memset, no floating-point atomics: every result is the
 * same from call to call and from stream to stream.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 */
#ifndef MINDDET_HIP_CN_H_
#define MINDDET_HIP_CN_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_CN_MAX_OBJS 1024            /* M: a sample's draw list / slots are staged in LDS */
#define MD_CN_LOSS_MAX_CHANNELS 160    /* Cp: a strip of 64 cells of head and grad is staged in LDS */
#define MD_CN_LOSS_STRIP 64            /* cells per workgroup of the dense pass (the workspace formula) */
#define MD_CN_LOSS_COUNT_CHUNK 16384   /* heat-map elements per workgroup of the count pass (the workspace formula) */

typedef struct md_cn_targets_attrs {
    float min_overlap; /* gaussian_radius's min_overlap (reference 0.7), inside (0, 1); widened to float64 as it is */
} md_cn_targets_attrs;

/* The targets of COCOHP.preprocess_fn for a batch.  Two launches.
 * in : boxes[B,G,4] f32 (x0, y0, x1, y1 in OUTPUT-MAP coordinates: the fp32 values the reference holds in `bbox` after the flip and the
 *      two affine_transform calls, dataset.py:339-342, before the clip), classes[B,G] i32 (the reference's 1-based category_id; < 1 or
 *      > C: a padding row, skipped), G <= M
 * out: hm[B,C,H,W] f32, ind[B,M] i32, reg_mask[B,M] u8, wh[B,M,2] f32, reg[B,M,2] f32 -- every element written, zeros included ;
 *      [workspace u8, 16-byte aligned: md_cn_assign_targets_workspace_bytes(B, M) bytes, at least 16 B M; without it the library's
 *      per-stream scratch pool serves]
 * extra: md_cn_targets_attrs, required.  C, H, W, M from the shapes; H, W >= 1.
 *
 * Per row k (dataset.py:343-359 as written, fp32 unless said otherwise):
 *   clip      x to [0, W - 1], y to [0, H - 1] (a NaN stays a NaN)
 *   used      h = y1 - y0 > 0 and w = x1 - x0 > 0 (false for a NaN) and 1 <= class <= C
 *   radius    max(0, (int) gaussian_radius((ceil h, ceil w), min_overlap)), term by term in float64 on the two integers; the third
 *             root is (b3 + sq3) / 2 as in the reference
 *   centre    ct = ((x0 + x1) / 2, (y0 + y1) / 2), ct_int its truncation
 *   hm        hm[class - 1] = the maximum over the used rows of the class of (float) exp(-(dx^2 + dy^2) / (2 s^2)), s = (2 radius + 1) / 6,
 *             in float64 for |dx|, |dy| <= radius around ct_int, 0 elsewhere
 *   row out   wh[k] = (w, h), ind[k] = ct_int.y W + ct_int.x, reg[k] = ct - ct_int, reg_mask[k] = 1
 *   slots     the slot of a row is its own index k (not a compacted rank): a skipped row leaves a zero slot; slots k >= G are zero
 * 2: G > M, an extent other than documented, H or W < 1, min_overlap outside (0, 1) or not finite, a workspace that is not 16-byte aligned.
 * 4: M > MD_CN_MAX_OBJS, an operand of 2^30 elements or more, B or C > 65535, a workspace smaller than documented. */
int md_cn_assign_targets(MD_AOT_ARGS);
int64_t md_cn_assign_targets_workspace_bytes(int64_t B, int64_t M);

typedef struct md_cn_loss_attrs {
    int32_t num_classes;                      /* C */
    int32_t off_hm, off_wh, off_reg;          /* first channel of each head; off_reg -1: no offset head */
    float hm_weight, wh_weight, off_weight;   /* reference 1, 0.1, 1 */
} md_cn_loss_attrs;

/* CenterNetLossCell.construct behind the network for a batch.  Three launches.
 * in : head[B,H,W,Cp] bf16 (raw logits: hm at off_hm .. + C, wh at off_wh .. + 2, reg at off_reg .. + 2; any other channel is padding
 *      whose value never enters the arithmetic), hm[B,C,H,W] f32, ind[B,M] i32, reg_mask[B,M] u8, wh[B,M,2] f32, reg[B,M,2] f32 (the
 *      outputs of md_cn_assign_targets)
 * out: parts[3] f32 (hm_loss, wh_loss, off_loss), num_pos[1] f32, total[1] f32 ;
 *      md_cn_loss_grad only: grad[B,H,W,Cp] f32 = d total / d head, every element written ;
 *      [workspace u8, 8-byte aligned: md_cn_loss_workspace_bytes(B, C, H, W) bytes (one function for both entry points), at least
 *      8 B (4 + 2 ceil(H W / MD_CN_LOSS_STRIP)) + 4 ceil(B C H W / MD_CN_LOSS_COUNT_CHUNK); without it the library's per-stream
 *      scratch pool serves]
 * extra: md_cn_loss_attrs, required.  B, H, W >= 1.
 *
 * As real-valued math on the given bf16 and fp32 values.  Arithmetic: every per-element term and every sum is evaluated in float64
 * and rounded once to fp32 on output (a choice: the reference's MindSpore fp32 kernels are not pinned by its source).
 *   p          clip(sigmoid(x), 1e-4, 1 - 1e-4) on the C hm channels (the Sigmoid cell the reference applies inside the network)
 *   num_pos    the cells with hm == 1 over the batch; N = 1 when num_pos == 0, else num_pos
 *   pos        sum over cells with hm == 1 of log(p) (1 - p)^2
 *   neg        sum over cells with hm < 1 of log(1 - p) p^2 (1 - hm)^4; a cell with hm > 1 or NaN is in neither sum
 *   hm_loss    -(pos + neg) / N
 *   valid slot reg_mask != 0 and 0 <= ind < H W.  Any other slot is skipped as if masked: its ind is never used as an address and
 *              it does not count (the reference would index out of range).  A non-zero mask counts as 1.
 *   wh_loss    sum over valid slots and j of |pred_j - wh_j| / (2 n_valid + 1e-4), pred read at cell ind from channels off_wh + j
 *   off_loss   the same on reg / off_reg; 0, with zero gradient, when off_reg == -1 or off_weight <= 0
 *   total      hm_weight hm_loss + wh_weight wh_loss + off_weight off_loss
 *   grad       the exact derivative of total, each element rounded to fp32 once.  hm channels: -hm_weight / N (1 - p)^2 ((1 - p) -
 *              2 p log p) where hm == 1, -hm_weight / N (1 - hm)^4 p^2 (2 (1 - p) log(1 - p) - p) where hm < 1, exactly +0 where the
 *              clip is active.  Regression channels: weight sign(pred - target) / (2 n_valid + 1e-4) summed over the valid slots at
 *              the cell, sign(0) = 0.  Padding channels and cells nothing touches: +0.
 * md_cn_loss and md_cn_loss_grad give bit-identical parts, num_pos and total.
 * 2: an extent other than documented, B, H or W < 1, a head outside [0, Cp) (off_reg < -1) or two heads sharing a channel,
 *    num_classes != C, a non-finite weight.
 * 4: M > MD_CN_MAX_OBJS, Cp > MD_CN_LOSS_MAX_CHANNELS, an operand of 2^30 elements or more, B > 65535, a workspace smaller than
 *    documented. */
int md_cn_loss(MD_AOT_ARGS);      /* forward only */
int md_cn_loss_grad(MD_AOT_ARGS); /* forward + d total / d head, in the same passes */
int64_t md_cn_loss_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_CN_H_ */
