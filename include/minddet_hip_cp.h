/*
 * minddet_hip_cp.h -- C ABI of the CenterPoint (CenterHead) post-processing of libminddet_hip.so for every task and every sample of a
 * batch: a batched rotated NMS, the scores of every BEV cell of every task in one pass over the head tensor, the box decode of the
 * selected cells only, and the task merge.  Chain: md_cp_scores -> md_topk_segmented (B T segments of n cells, min_score -1,
 * max_segment n) -> md_cp_decode_selected -> md_nms_rotated (mode 1, max_output = nms_post_max_size) -> md_cp_pack; nothing is read
 * back by the host in between.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions"), which this header includes.
 *
 * The head ops read the head tensor of the model in place: head[B,H,W,C] bf16 (NHWC) holds, per cell (y, x), the outputs of every
 * task's SepHead branches (minddet/models/centerpoint/det3d_ms/models/bbox_heads/center_head.py:28-99) side by side, task t's heads
 * at the channels md_cp_head_attrs.task[t] names.  The cell index within a sample is y * W + x, n = H * W cells; T = num_tasks,
 * k = the rows the top-k selected per (sample, task) (nms_pre_max_size), m = max_per_task (nms_post_max_size).
 */
#ifndef MINDDET_HIP_CP_H_
#define MINDDET_HIP_CP_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_CP_MAX_TASKS 8

typedef struct md_nms_rotated_attrs {
    float iou_threshold;
    int32_t mode;       /* 0: the NmsGpu rule, suppress iff so / fmaxf(sa + sb - so, 1e-8) > iou_threshold;
                           1: the boxes_iou_nms_cpu rule, suppress iff so / (sa + sb - so) >= iou_threshold, and boxes of area 0 are
                              removed up front without suppressing anything (iou-bev-nms-org.cpp:250-256) */
    int32_t max_output; /* > 0: stop after this many kept boxes per list; 0: no quota */
} md_nms_rotated_attrs;

/* Greedy rotated-BEV NMS over L score-sorted lists in one call: NmsGpu (centerpoint/det3d_ms/ops/iou3d_nms/src/iou3d_nms_kernel.cu:
 * 267-372, iou3d_nms.cpp:102-133) or boxes_iou_nms_gpu (centerpoint/det3d_ms/ops/iou-bev-nms-org.cpp:237-283) per list, in the shape
 * of md_nms_aligned.
 * in : boxes[L,N,7] f32 (x, y, z, dx, dy, dz, heading; or [N,7], L = 1), count[L] i32 or NULL (all N rows of every list valid)
 * out: keep_idx[L,N] i32 (the leading num[l] entries are the kept rows in order, the rest 0), num[L] i32 ; [workspace u8:
 *      md_nms_rotated_workspace_bytes(L, N) bytes, at least L N (20 x 4 + ceil(N / 64) x 8); without it the library's per-stream
 *      scratch pool serves]
 * extra: md_nms_rotated_attrs, required.
 * Only the first min(count[l], N) rows of list l are read (a count <= 0 keeps nothing).  The per-pair predicate is the one the
 * single-list operators compute, so keep_idx[l, :num[l]] equals NmsGpu / boxes_iou_nms_gpu on boxes[l, :count[l]] bit for bit (cut
 * to max_output where given).
 * 2: the last extent of boxes != 7, count / keep_idx / num not of L / L N / L elements, mode outside {0, 1}, max_output < 0.
 * 4: N > 65536 or L > 65535, a workspace smaller than documented. */
int md_nms_rotated(MD_AOT_ARGS);
int64_t md_nms_rotated_workspace_bytes(int64_t L, int64_t n);

typedef struct md_cp_task_attrs {
    int32_t off_reg, off_height, off_dim, off_rot; /* first channel of the task's reg (2), height (1), dim (3), rot (2) heads */
    int32_t off_vel;                               /* first channel of vel (2); -1: the task has none (velocities are 0) */
    int32_t off_hm;                                /* first channel of the heat map (num_classes channels) */
    int32_t num_classes;
    int32_t class_base;                            /* md_cp_pack: added to the task-local label (the summed num_classes of the earlier tasks) */
} md_cp_task_attrs;

typedef struct md_cp_head_attrs {
    int32_t num_tasks; /* T, 1 .. MD_CP_MAX_TASKS */
    md_cp_task_attrs task[MD_CP_MAX_TASKS];
    float score_threshold, out_size_factor;
    float voxel_size[2], pc_range[2], post_center_range[6];
    int32_t max_per_task; /* m = nms_post_max_size (md_cp_pack) */
} md_cp_head_attrs;

/* CenterHead.predict + post_processing up to the mask (center_head.py:297-334, 408-423), every task in one pass over the head tensor.
 * in : head[B,H,W,C] bf16
 * out: scores[B,T,n] f32
 * extra: md_cp_head_attrs, required (num_tasks, the tasks' offsets and num_classes, score_threshold .. post_center_range are read).
 * Per cell and task, in fp32 and with the arithmetic of md_centerpoint_decode (the same device function, so the two agree bit for
 * bit): best = the first maximum of 1 / (1 + expf(-hm_c)); xs = (x + reg_0) out_size_factor voxel_size[0] + pc_range[0], ys likewise,
 * zs = height; score = best where best > score_threshold and (xs, ys, zs) lies inside post_center_range (bounds included), else -1.
 * 2: num_tasks outside 1 .. 8, num_classes < 1, a head's channels not inside [0, C) (off_vel < -1), scores not [B,T,n].
 * 4: H or W > 65536, C > 480, B T n or B H W C >= 2^31. */
int md_cp_scores(MD_AOT_ARGS);

/* The box decode of the selected cells only (center_head.py:310-334, the NMS operand of :426-430).
 * in : head[B,H,W,C] bf16, idx[B,T,k] i32 (cell index within the sample: md_topk_segmented's indices), cnt[B,T] i32 (valid leading
 *      rows, clamped to k)
 * out: boxes[B,T,k,9] f32 (x, y, z, dx, dy, dz, vx, vy, rot), nms_boxes[B,T,k,7] f32 (x, y, z, dy, dx, dz, -rot - pi/2),
 *      labels[B,T,k] i32 (the task-local first arg-max of the heat map, recomputed by the device function md_cp_scores uses)
 * extra: md_cp_head_attrs, required (as md_cp_scores; the thresholds are not applied: a selected cell has passed them).
 * Rows j >= cnt[b,t] are all zero.  idx lives on the device, so it cannot be checked here: a row whose index is outside [0, n) is
 * written as zeros too and nothing is read for it.
 * 2: as md_cp_scores, and idx not [B,T,k], cnt not [B,T], an output's extents other than documented.
 * 4: H or W > 65536, B T k x 9 or B H W C >= 2^31. */
int md_cp_decode_selected(MD_AOT_ARGS);

/* count = min(num_out, mask_num, nms_post_max_size) (center_head.py:455-458) and the task merge of tools_ms/eval.py:84-111.
 * in : boxes[B,T,k,9] f32, sel_scores[B,T,k] f32 (the top-k's values), labels[B,T,k] i32, keep_idx[B,T,k] i32 and num[B,T] i32
 *      (md_nms_rotated's outputs), cnt[B,T] i32 (the top-k's counts)
 * out: dets[B,T m,11] f32 (the 9 box values, score, label), count[B] i32
 * extra: md_cp_head_attrs, required (num_tasks, max_per_task and every task's class_base are read).
 * Per sample, tasks in order: c = min(num, cnt, m, k); size = the number of j < c with sel_scores[keep_idx[j]] > 0; the rows
 * keep_idx[0 .. size) of the task are appended as (boxes row, its score, (float)(label + class_base)).  count[b] = the rows appended;
 * every row of dets past it is written as zeros (no separate clear is needed).  A keep_idx outside [0, k) gives a zero row.
 * 2: num_tasks outside 1 .. 8 or != T, max_per_task < 0, an operand's extents other than documented.
 * 4: B T k x 9 or B T m x 11 >= 2^31, T m > 65536. */
int md_cp_pack(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_CP_H_ */
