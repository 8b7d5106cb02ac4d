/*
 * minddet_hip_kittieval.h -- C ABI of the KITTI AP evaluation of libminddet_hip.so: from packed annotations (or the result rows
 * md_kitti_rows wrote) to the [class, difficulty, overlap level, 41] count tables.  What it replaces, host numpy / numba in the
 * reference: clean_data, image_box_overlap / bev_box_overlap / d3_box_overlap, compute_statistics, get_thresholds and the sums of
 * eval_class (pointpillars/eval_gpu/eval.py:9-27, 30-87, 91-162, 166-297, 483-599; pointpillars/src/core/eval_utils.py:36-115 for the
 * "ms" table), with rotate_iou_kernel_eval (eval_gpu/rotate_iou.py:167-302) for the rotated pairs.  minddet_amd/kitti_eval.py states
 * the same rules on the host and is the judge of these operators; the divisions and the right-to-left envelope of eval_class stay on
 * the host, on the count tables.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 *
 * No random number generator, no floating-point atomics, no memset, no host read, no workspace and no use of the scratch pool: every
 * intermediate buffer is a named output operand sized from extents the host knows, and two calls give the same bits.  No output may
 * share its address with an input or with another output: such a call is refused with rc 2.  Every decision is evaluated in float64
 * from the operands without contraction, in the order kitti_eval.py writes the operations; a value is rounded once, where it is
 * stored.  The one fp32 island is the rotated pair arithmetic of metrics 1 and 2, which is md_rotate_iou_eval's (csrc/rot_eval.h).
 *
 * Packed layout (kitti_eval.pack_annos), I images, Gt ground-truth rows, Dt detection rows, Cn classes of one evaluation:
 *   gt_off[I+1] i32, dt_off[I+1] i32: image i owns the rows [off[i], off[i+1]); G_i and D_i are their differences
 *   ov_off[I+1] i64: ov_off[i] = sum over j < i of G_j D_j; image i's overlap block is ground-truth-major [G_i, D_i]
 *   gt_box[Gt,4] f64, gt_alpha[Gt] f64, gt_occ[Gt] i32, gt_trunc[Gt] f64, gt_cam[Gt,7] f64 (x, y, z, l, h, w, ry),
 *   gt_dc[Gt] u8 (1: the name is "DontCare"), gt_valid[Cn,Gt] u8 (1 + clean_data's valid: 0 other, 1 neighbour class, 2 the class)
 *   dt_box[Dt,4] f64, dt_alpha[Dt] f64, dt_score[Dt] f64, dt_cam[Dt,7] f64, dt_same[Cn,Dt] u8 (1: the detection's name is the class)
 * Flags travel as u8 = 1 + the flag of clean_data: 0 other class (-1), 1 counted (0), 2 ignored (1).
 * Tasks are (class c, difficulty d of 3, overlap level k of K), task = (c 3 + d) K + k.
 *
 * Limits.  The host checks what the extents say: I, Cn, K, the element count of ov, and Gt / Dt against I times the per-image limit.
 * G_i and D_i themselves are device data: the kernels clamp them to the limit and skip an image whose offsets leave its operands (so
 * nothing is read or written out of bounds); the Python layer (kitti_eval.pack_annos, det_ops) raises ValueError before any call.
 */
#ifndef MINDDET_HIP_KITTIEVAL_H_
#define MINDDET_HIP_KITTIEVAL_H_

#include "minddet_hip_kitti.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_KEVAL_MAX_DETS 512      /* D_i: detections per image (MD_KITTI_MAX_DETS of the rows) */
#define MD_KEVAL_MAX_GTS 512       /* G_i: ground-truth rows per image */
#define MD_KEVAL_MAX_IMAGES 65536  /* I */
#define MD_KEVAL_MAX_CLASSES 8     /* Cn */
#define MD_KEVAL_MAX_LEVELS 4      /* K: overlap levels */
#define MD_KEVAL_SAMPLE_PTS 41     /* N_SAMPLE_PTS */

typedef struct md_kitti_eval_flags_attrs {
    int32_t abs_gt_height; /* 0 or 1; 1: the ground-truth height is abs(y2 - y1) (eval_utils.py:49, the "ms" table); 0: eval_gpu/eval.py:44 */
} md_kitti_eval_flags_attrs;
/* clean_data for the three difficulties and Cn classes.
 * in : gt_box[Gt,4] f64, gt_occ[Gt] i32, gt_trunc[Gt] f64, gt_valid[Cn,Gt] u8, dt_box[Dt,4] f64, dt_same[Cn,Dt] u8
 * out: ign_gt[Cn,3,Gt] u8, ign_dt[Cn,3,Dt] u8, num_valid[Cn,3] i32 (the counted ground truths, an integer block sum)
 * extra: md_kitti_eval_flags_attrs, required.
 * Difficulty d: MIN_HEIGHT 40 / 25 / 25, MAX_OCCLUSION 0 / 1 / 2, MAX_TRUNCATION 0.15 / 0.3 / 0.5.  Ground truth: height = y2 - y1;
 * ignore = occ > MAX_OCCLUSION or trunc > MAX_TRUNCATION or height <= MIN_HEIGHT; flag 0 if valid == 1 and not ignore, 1 if valid == 0
 * or (ignore and valid == 1), else -1.  Detection: flag 1 if abs(y2 - y1) < MIN_HEIGHT, else 0 if dt_same, else -1.
 * 2: an extent other than documented, abs_gt_height not 0 / 1, aliasing.  4: Cn > MD_KEVAL_MAX_CLASSES, Gt > MD_KEVAL_MAX_IMAGES
 * MD_KEVAL_MAX_GTS, Dt > MD_KEVAL_MAX_IMAGES MD_KEVAL_MAX_DETS. */
int md_kitti_eval_flags(MD_AOT_ARGS);

typedef struct md_kitti_eval_overlaps_attrs {
    int32_t metric; /* 0 image boxes, 1 BEV, 2 3D */
} md_kitti_eval_overlaps_attrs;
/* calculate_overlaps for all images in one launch, one lane per pair (a lane finds its image by a binary search of ov_off).
 * in : gt_off[I+1] i32, dt_off[I+1] i32, ov_off[I+1] i64, gt[Gt,W] f64, dt[Dt,W] f64: W = 4, the image boxes, for metric 0; W = 7,
 *      the camera boxes gt_cam / dt_cam, for metrics 1 and 2
 * out: ov[P] f64, P >= ov_off[I]: image i's block [G_i, D_i] at ov_off[i]; elements from ov_off[I] on are zero
 * extra: md_kitti_eval_overlaps_attrs, required.
 * Metric 0: image_box_overlap(dt, gt): iw = min(x2) - max(x1), ih alike, inter = iw ih, inter / ((a + q) - inter) with a the
 * detection's area, 0 where iw <= 0 or ih <= 0.  Metric 1: rotate_iou_kernel_eval, criterion -1, on (x, z, l, w, ry) rounded to fp32,
 * the detection as the box and the ground truth as the query box, widened to float64.  Metric 2: the same kernel's criterion 2 (rinc),
 * then d3_box_overlap in float64: ih = min(y) - max(y - h), inc = ih rinc, inc / ((v1 + v2) - inc) where rinc > 0 and ih > 0, 0 where
 * only rinc > 0, rinc otherwise (np.where(rinc > 0, out, rinc)).
 * 2: an extent other than documented, a metric outside 0 .. 2, aliasing.  4: I > MD_KEVAL_MAX_IMAGES, P >= 2^31, Gt or Dt as above. */
int md_kitti_eval_overlaps(MD_AOT_ARGS);

/* Pass 1 of eval_class: compute_statistics(compute_fp=False, thresh 0) for every (task, image), one wave each.
 * in : ov[P] f64, ign_gt[Cn,3,Gt] u8, ign_dt[Cn,3,Dt] u8, dt_score[Dt] f64, gt_off[I+1] i32, dt_off[I+1] i32, ov_off[I+1] i64,
 *      min_overlap[Cn,K] f64
 * out: matched[Cn,3,K,Gt] f64: the score of the detection that became a true positive for the ground truth, -inf otherwise
 * Ground truths in order; one with flag -1 is skipped.  Candidates: detections with flag != -1, not assigned, ov > min_overlap.  The
 * winner is the highest score, the lowest index on equal scores; it is marked assigned; it counts (its score is stored) unless the
 * ground truth or the detection is ignored.
 * 2: an extent other than documented, aliasing.  4: I, Cn, Gt, Dt, P as above, K > MD_KEVAL_MAX_LEVELS. */
int md_kitti_eval_match(MD_AOT_ARGS);

/* get_thresholds for every task, one lane each: the recurrence itself in float64.
 * in : sorted[Cn,3,K,Gt] f64: the rows of matched sorted descending (the -inf tail last); num_valid[Cn,3] i32
 * out: thresholds[Cn,3,K,41] f64 (NaN behind nthresh), nthresh[Cn,3,K] i32
 * For i over the n finite-or-+inf leading scores: l = (i + 1) / num_gt, r = (i + 2) / num_gt (l for the last); skipped when
 * (r - current) < (current - l) and i < n - 1; else the score is a threshold and current += 1 / 40.0.  At most 41 are stored.
 * 2: an extent other than documented, aliasing.  4: Cn, K, Gt as above. */
int md_kitti_eval_thresholds(MD_AOT_ARGS);

typedef struct md_kitti_eval_stats_attrs {
    int32_t metric;      /* 0, 1, 2: the DontCare discount applies to metric 0 only */
    int32_t compute_aos; /* 0 or 1 */
} md_kitti_eval_stats_attrs;
/* Pass 2 of eval_class: compute_statistics(compute_fp=True) for every (task, threshold < nthresh, image), one wave per (task, image)
 * looping over the thresholds, then the sums over the images in a second launch, in image order.
 * in : ov[P] f64, ign_gt[Cn,3,Gt] u8, ign_dt[Cn,3,Dt] u8, dt_score[Dt] f64, gt_off[I+1] i32, dt_off[I+1] i32, ov_off[I+1] i64,
 *      min_overlap[Cn,K] f64, thresholds[Cn,3,K,41] f64, nthresh[Cn,3,K] i32, gt_box[Gt,4] f64, gt_dc[Gt] u8, dt_box[Dt,4] f64,
 *      gt_alpha[Gt] f64, dt_alpha[Dt] f64
 * out: img_counts[Cn,3,K,41,I,3] i32 (tp, fp, fn), img_sim[Cn,3,K,41,I] f64, pr_counts[Cn,3,K,41,3] i32, pr_sim[Cn,3,K,41] f64.
 *      Every element is written on every call; rows at or behind nthresh are zero.
 * extra: md_kitti_eval_stats_attrs, required.
 * Per ground truth in order (flag -1 skipped): candidates as in pass 1 minus detections with score < thresh; among the counted
 * candidates (flag 0) the largest overlap wins, the lowest index on ties; otherwise the first ignored candidate (flag 1).  No
 * winner: fn + 1 if the ground truth is counted.  A winner is assigned; it is a true positive unless it or the ground truth is
 * ignored.  fp = detections that are unassigned, flag 0, not below the threshold and, on metric 0, not inside a DontCare box:
 * image_box_overlap(det, dc, criterion 0) = inter / (a + 0 q) > min_overlap for one of the image's gt_dc rows.  img_sim = the sum over
 * the image's true positives in ground-truth order of (1 + cos(gt_alpha - dt_alpha)) / 2 when compute_aos, else 0; pr_sim adds the
 * images in order from 0.
 * 2: an extent other than documented, metric outside 0 .. 2, compute_aos not 0 / 1, aliasing.  4: I, Cn, K, Gt, Dt, P as above. */
int md_kitti_eval_stats(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_KITTIEVAL_H_ */
