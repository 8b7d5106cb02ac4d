/*
 * minddet_hip_cptargets.h -- C ABI of the CenterPoint training targets of libminddet_hip.so: the AssignLabel pipeline step
 * (minddet/models/centerpoint/det3d_ms/datasets/pipelines/preprocess.py:285-521, with gaussian_radius / gaussian2D / draw_umich_gaussian
 * of det3d_ms/core/utils/center_utils.py:16-65 and limit_period of det3d_ms/core/bbox/box_np_ops.py:247-248) for every task and every
 * sample of a batch, on the grid and with the per-task class bookkeeping of md_cp_scores / md_cp_decode_selected (minddet_hip_cp.h).
 * Two launches, no host read, no atomics: the result is deterministic.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions"), which this header includes.
 */
#ifndef MINDDET_HIP_CPTARGETS_H_
#define MINDDET_HIP_CPTARGETS_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_CP_TARGETS_MAX_TASKS 8
#define MD_CP_TARGETS_MAX_GT 1024

typedef struct md_cp_targets_attrs {
    int32_t num_tasks;       /* T, 1 .. MD_CP_TARGETS_MAX_TASKS */
    int32_t num_classes[8];  /* per task, >= 1; task t owns the global classes (sum of the earlier tasks') + 1 .. + num_classes[t] */
    float voxel_size[2];     /* x, y; > 0 */
    float pc_range[2];       /* lower x, y of the range */
    int32_t out_size_factor; /* > 0 */
    float gaussian_overlap;  /* in (0, 1) */
    int32_t min_radius;      /* >= 0 */
} md_cp_targets_attrs;

/* AssignLabel.__call__ (preprocess.py:297-521, the NuScenesDataset branch) for a batch.
 * in : gt_boxes[B,G,9] f32 (x, y, z, w, l, h, vx, vy, rot), gt_classes[B,G] i32 (global 1-based class; 0, a negative id or an id past
 *      the last task's classes: a padding row that belongs to no task)
 * out: hm[B,T,C,H,W] f32 (C = the largest num_classes; row = y, column = x), anno_box[B,T,M,10] f32, ind[B,T,M] i32, mask[B,T,M] u8,
 *      cat[B,T,M] i32, gt_boxes_and_cls[B,M,10] f32 ; [workspace u8: md_cp_assign_targets_workspace_bytes(B, T, G) bytes, at least
 *      B T (G + 1) x 16; without it the library's per-stream scratch pool serves]
 * extra: md_cp_targets_attrs, required.  M = max_objs and the feature map H x W are taken from the shapes.
 * Every element of every output is written (zeros included): the caller clears nothing.
 *
 * Per sample, in the reference's arithmetic under NumPy >= 2 scalar promotion (fp32 scalars; fp contraction off, fp32 divides and
 * square roots correctly rounded):
 *   membership  task t owns the rows whose class lies in its range; inside a task the rows are ordered by class, then by original
 *               index (np.where per class name + concatenate, :323-351); slot k is that rank.  Unused slots and the slots of skipped
 *               rows are zero with mask 0.
 *   heading     rot <- rot - floor(rot / P + 0.5) * P, P = (float)(2 pi) (limit_period(rot, 0.5, 2 pi), :353-357); anno_box and
 *               gt_boxes_and_cls both carry the wrapped heading (the reference writes it back in place).
 *   cells       w / voxel_size[0] / out_size_factor, l / voxel_size[1] / out_size_factor, ct = (x - pc_range[0]) / voxel_size[0] /
 *               out_size_factor (y likewise): two successive divides each.  ct_int = truncation.  A row is skipped when w <= 0 or
 *               l <= 0 in cells, when ct_int lies outside [0, W) x [0, H), or when ct is not finite.
 *   radius      gaussian_radius((l, w), gaussian_overlap) term by term (center_utils.py:16-36, the third root as (b3 + sq3) / 2),
 *               radius = max(min_radius, (int)radius).  A radius of 1e9 cells or more is outside the contract.
 *   heat map    hm[t, class] = the maximum over the task's drawn rows of that class of (float)exp(-(dx dx + dy dy) / (2 s s)),
 *               s = (2 radius + 1) / 6, evaluated in float64 for the integer offsets |dx|, |dy| <= radius from ct_int; 0 where no
 *               Gaussian reaches, exactly 1 in a centre cell.
 *   row at its slot   cat = class within the task (0-based), ind = y W + x of ct_int, mask = 1,
 *               anno_box = (ct - ct_int (2), z, log w, log l, log h, vx, vy, sin rot, cos rot)
 *   gt_boxes_and_cls  the rows that belong to a task (skipped ones included), by task, then slot: (x, y, z, w, l, h, rot, vx, vy,
 *               (float)global class) (:484-503); the remaining rows are zero.
 * 2: G > M (the reference's assertion, :500), an extent other than documented, C != max(num_classes), num_tasks outside 1 .. 8,
 *    num_classes < 1, voxel_size / out_size_factor not positive, gaussian_overlap outside (0, 1), min_radius < 0, a non-finite attribute.
 * 4: G > MD_CP_TARGETS_MAX_GT (the rows of a sample are staged in LDS), an operand of 2^30 elements or more, B or T C > 65535,
 *    a workspace smaller than documented. */
int md_cp_assign_targets(MD_AOT_ARGS);
int64_t md_cp_assign_targets_workspace_bytes(int64_t B, int64_t T, int64_t G);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_CPTARGETS_H_ */
