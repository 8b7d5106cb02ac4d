/*
 * minddet_hip_cploss.h -- C ABI of the CenterPoint training loss of libminddet_hip.so: CenterHead.loss
 * (minddet/models/centerpoint/det3d_ms/models/bbox_heads/center_head.py:208-271) with FastFocalLoss and RegLoss
 * (det3d_ms/models/losses/centernet_loss.py:22-82) for every task of a batch, on the merged head tensor of md_cp_scores
 * (minddet_hip_cp.h) and the targets of md_cp_assign_targets (minddet_hip_cptargets.h).  Three launches, no host read, no memset, no
 * atomics: the result is the same from call to call and from stream to stream.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 */
#ifndef MINDDET_HIP_CPLOSS_H_
#define MINDDET_HIP_CPLOSS_H_

#include "minddet_hip_cp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_CP_LOSS_MAX_OBJS 1024     /* M: a (sample, task)'s slots are staged in LDS */
#define MD_CP_LOSS_MAX_CHANNELS 160  /* Cp: a strip of 64 cells of head and grad is staged in LDS */
#define MD_CP_LOSS_STRIP 64          /* cells per workgroup of the dense pass (the workspace formula) */

typedef struct md_cp_loss_attrs {
    int32_t num_tasks;                      /* T, 1 .. MD_CP_MAX_TASKS */
    md_cp_task_attrs task[MD_CP_MAX_TASKS]; /* the heads' first channels and num_classes; class_base is not read */
    float weight;                           /* loc-loss weight (reference default 0.25) */
    float code_weights[10];                 /* order of anno_box: reg 2, height 1, dim 3, vel 2, rot 2 */
} md_cp_loss_attrs;

/* CenterHead.loss for a batch.
 * in : head[B,H,W,Cp] bf16 (raw logits; task t's heads at the channels task[t] names, any channel no head owns is padding: its value
 *      never enters the arithmetic), hm[B,T,C,H,W] f32, anno_box[B,T,M,10] f32, ind[B,T,M] i32, mask[B,T,M] u8, cat[B,T,M] i32 (the outputs of
 *      md_cp_assign_targets; C = the largest num_classes)
 * out: parts[T,12] f32 (per task hm_loss, loc_loss, box_loss[10]), num_pos[T] f32, total[1] f32 ;
 *      md_cp_loss_grad only: grad[B,H,W,Cp] f32 = d total / d head, every element written (zeros and padding channels included) ;
 *      [workspace u8: md_cp_loss_workspace_bytes(B, T, H, W) bytes (one function for both entry points), at least
 *      8 B T (12 + ceil(H W / MD_CP_LOSS_STRIP)); without it the library's per-stream scratch pool serves]
 * extra: md_cp_loss_attrs, required.  B, H, W >= 1.
 *
 * Per task t, as real-valued math on the given bf16 and fp32 values.  Arithmetic: every per-element term and every sum is evaluated
 * in float64 and rounded once to fp32 on output (a choice: the reference's MindSpore fp32 kernels are not pinned by its source; the
 * literal fp32 log(1 - p) would be off by up to 1.2e-4 relative on the gradient for small p).
 *   p           clip(sigmoid(x), 1e-4, 1 - 1e-4) (float64 bounds) on the task's num_classes hm channels.  Target planes
 *               c >= num_classes[t] of hm are never read.
 *   valid slot  mask != 0 and 0 <= ind < H W and 0 <= cat < num_classes[t].  Any other slot is skipped as if masked: its ind / cat are
 *               never used as an address and it does not count in num_pos (the reference would index out of range).
 *   num_pos     the valid slots over the whole batch
 *   neg         sum over b, c, y, x of log(1 - p) p^2 (1 - hm)^4
 *   pos         sum over valid slots of log(p_s) (1 - p_s)^2, p_s = p at (b, ind, cat)
 *   hm_loss     -neg when num_pos == 0, else -(pos + neg) / num_pos
 *   box_loss[j] sum over valid slots of |pred_j - target_j| / (num_pos + 1e-4), pred read at the cell ind.  Column j of anno_box is
 *               (reg 0-1, height, dim 0-2, vel 0-1, rot 0-1); the head channel of each comes from the task's offsets (the head stores
 *               rot before vel).  A task with off_vel == -1 compares (reg, height, dim, rot) with target columns 0..5, 8, 9 under the
 *               first 8 code weights (center_head.py:239-250); its box_loss[8..9] are 0.
 *   loc_loss    sum over j of box_loss[j] code_weights[j]
 *   total       sum over t of hm_loss + weight loc_loss
 *   grad        the exact derivative of total.  hm channels: scale ((1 - hm)^4 p^2 (2 (1 - p) log(1 - p) - p) + sum over the valid
 *               slots at this (cell, class) of (1 - p)^2 ((1 - p) - 2 p log p)), scale = -1 / num_pos (-1 when num_pos == 0); exactly
 *               0 where the clip is active (sigmoid(x) outside (1e-4, 1 - 1e-4)).  Regression channels: weight code_weights[j]
 *               sign(pred - target) / (num_pos + 1e-4) summed over the valid slots at the cell, sign(0) = 0.  Slots that share a
 *               cell, or a cell and a class, add up; each element is rounded to fp32 once, from the float64 sum.
 * md_cp_loss and md_cp_loss_grad give bit-identical parts, num_pos and total.
 * 2: an extent other than documented, B, H or W < 1, num_tasks outside 1 .. 8 or != T, num_classes < 1, C != max(num_classes), a head's
 *    channels not inside [0, Cp) (off_vel < -1) or two heads sharing a channel, a non-finite weight or code weight.
 * 4: M > MD_CP_LOSS_MAX_OBJS, Cp > MD_CP_LOSS_MAX_CHANNELS, an operand of 2^30 elements or more, B > 65535, a workspace smaller than
 *    documented. */
int md_cp_loss(MD_AOT_ARGS);      /* forward only */
int md_cp_loss_grad(MD_AOT_ARGS); /* forward + d total / d head, in the same passes */
int64_t md_cp_loss_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t W);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_CPLOSS_H_ */
