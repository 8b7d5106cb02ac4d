/*
 * minddet_hip_nusceval.h -- C ABI of the nuScenes detection evaluation (detection_cvpr_2019) of libminddet_hip.so: from the fixed-shape
 * output of CenterPoint (md_cp_pack: dets [B, max_det, 11], count [B]) and packed ground truth to the precision [Kc, D, R], confidence
 * [Kc, D, R] and true-positive error [Kc, 5, R] curves that the devkit's DetectionEval computes.  What it replaces, host Python in the
 * reference: _second_det_to_nusc_box and _lidar_nusc_box_to_global (centerpoint/det3d_ms/datasets/nuscenes/nusc_common.py:160-201), the
 * attribute rule of nuscenes.py:252-293 and the DetectionEval called from nusc_common.py:659-674.  minddet_amd/nusc_eval.py states the same
 * rules on the host (dets_to_nusc, NuscDetectionEval) and is the judge of these operators; AP, the TP metrics, mAP and NDS (summarize())
 * stay on the host, on the three tables.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 *
 * No random number generator, no floating-point atomics, no memset, no host read, no workspace and no use of the scratch pool: every
 * intermediate buffer is a named output operand sized from extents the host knows, and two calls give the same bits.  No output may
 * share its address with an input or with another output: such a call is refused with rc 2.  Every decision is evaluated in float64
 * from the operands without contraction, in the order nusc_eval.py writes the operations; a value is rounded once, where it is stored.
 * sqrt, division and fmod are correctly rounded; sin, cos and atan2 (dt_quat, dt_yaw) are the device's and are held to an interval.
 *
 * Packed layout (nusc_eval.pack_nusc).  I samples in order, Kc classes, cell c = i Kc + k; D distance thresholds (4), R recall points
 * (101); Gt ground-truth rows, Dt detection rows.  Quaternions are (w, x, y, z).
 *   gt_beg, gt_cnt, dt_beg, dt_cnt [I Kc] i32: a cell owns the rows [beg, beg + cnt).  "Begin + count" so that a compact host packing and
 *     the padded per-sample layout of md_nusc_rows both fit; rows outside every cell are never read.
 *   gt_xy[Gt,2], gt_size[Gt,3], gt_yaw[Gt], gt_vel[Gt,2] f64 (NaN: unknown), gt_attr[Gt] i32 (the attribute code, -1 for none); a cell's
 *     ground truths are in record order.
 *   dt_xyz[Dt,3], dt_size[Dt,3], dt_quat[Dt,4], dt_vel[Dt,2], dt_yaw[Dt], dt_score[Dt] f64, dt_cat[Dt] i32 (k, or Kc for an unused row),
 *     dt_attr[Dt] i32, dt_rank[Dt] i32 (the place inside the cell), dt_src[Dt] i32.  A cell's detection rows are in walking order:
 *     descending score, on equal scores the higher source row first (the devkit's sorted(...)[::-1]).
 *   dist_thr[D] f64 ascending or not, period[Kc] f64 (pi for barrier, 2 pi otherwise), rec_thr[R] f64 (linspace(0, 1, 101)).
 *
 * Limits.  The host checks what the extents say (rc 4).  The per-cell counts are device data: the kernels clamp them to the limit and
 * skip a cell whose rows leave the operands (so nothing is read or written out of bounds); the Python layer (nusc_eval.pack_nusc,
 * PackedNusc.add_dets, det_ops) raises ValueError before any call.
 */
#ifndef MINDDET_HIP_NUSCEVAL_H_
#define MINDDET_HIP_NUSCEVAL_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_NUSCEVAL_MAX_SAMPLE_DETS 512 /* max_det: detection rows per sample (and so per cell) */
#define MD_NUSCEVAL_MAX_GTS 1024        /* ground truths per cell */
#define MD_NUSCEVAL_MAX_CLASSES 16      /* Kc */
#define MD_NUSCEVAL_MAX_THRS 8          /* D */
#define MD_NUSCEVAL_MAX_RECS 256        /* R */
#define MD_NUSCEVAL_MAX_CELLS 16777216  /* I Kc stays below this (2^24) */
#define MD_NUSCEVAL_MAX_ROWS 67108864   /* Gt, Dt (2^26) */
#define MD_NUSCEVAL_MAX_LABELS 4096     /* L: entries of label_to_k */

typedef struct md_nusc_rows_attrs {
    int32_t first_sample; /* the batch's first sample: batch entry b writes the rows and cells of sample first_sample + b */
} md_nusc_rows_attrs;
/* dets_to_nusc, the class-range filter and the grouping into cells for one batch, nothing read back; one workgroup per sample, rank by
 * counting.
 * in : dets[B,max_det,11] f32 (x, y, z, dx, dy, dz, vx, vy, rot, score, label), count[B] i32, pose[B,14] f64 (cs_rotation, cs_translation,
 *      ego_rotation, ego_translation), label_to_k[L] i32 (-1 drops the row), class_range[Kc] f64, attr_moving[Kc] i32, attr_still[Kc] i32
 * out: dt_xyz[Dt,3], dt_size[Dt,3], dt_quat[Dt,4], dt_vel[Dt,2], dt_yaw[Dt], dt_score[Dt] f64, dt_cat[Dt], dt_attr[Dt], dt_rank[Dt],
 *      dt_src[Dt] i32 (the source row, -1 for an unused one), dt_beg[I Kc], dt_cnt[I Kc] i32; Dt = I max_det.  Sample i owns the rows
 *      [i max_det, (i + 1) max_det) and the cells [i Kc, (i + 1) Kc); the call writes every element of the samples first_sample ..
 *      first_sample + B - 1 and nothing else.
 * extra: md_nusc_rows_attrs, required.
 * Row r < min(count, max_det): yaw' = (-rot) - (float)(pi / 2) in float32; h = (double)yaw' / 2, q = (cos h, 0, 0, sin h); c = (x, y, z),
 * v = (vx, vy, 0) widened; then twice (cs, ego): c = R(rot) c + translation, q = rot q (Hamilton, rot as given), v = R(rot) v, with R the
 * matrix of the normalised quaternion: n = sqrt(((w w + x x) + y y) + z z), components / n, r00 = 1 - 2 (y y + z z), r01 = 2 (x y - w z),
 * r02 = 2 (x z + w y), r10 = 2 (x y + w z), r11 = 1 - 2 (x x + z z), r12 = 2 (y z - w x), r20 = 2 (x z - w y), r21 = 2 (y z + w x),
 * r22 = 1 - 2 (x x + y y); R u = ((r0 ux + r1 uy) + r2 uz) per row.  dt_yaw = atan2(r10, r00) of R(q); size = dets[3:6] as it lies.
 * The row is taken when its label l (truncated) lies in [0, L), 0 <= k = label_to_k[l] < Kc, its score is not NaN and
 * sqrt(ex ex + ey ey) < class_range[k] with e = c - ego_translation.  dt_attr = attr_moving[k] if sqrt(vx vx + vy vy) > 0.2 of the global
 * velocity, else attr_still[k].  The place of a row inside its sample is its rank under the key (k, score descending, source row
 * descending).  Unused rows: every float 0, dt_cat Kc, dt_attr 0, dt_rank 0, dt_src -1.
 * 2: an extent other than documented (Dt not I max_det, cells not I Kc), first_sample < 0 or first_sample + B > I, aliasing.
 * 4: max_det > MD_NUSCEVAL_MAX_SAMPLE_DETS, L > MD_NUSCEVAL_MAX_LABELS, Kc > MD_NUSCEVAL_MAX_CLASSES, cells >= MD_NUSCEVAL_MAX_CELLS,
 * Dt > MD_NUSCEVAL_MAX_ROWS. */
int md_nusc_rows(MD_AOT_ARGS);

typedef struct md_nusc_eval_attrs {
    int32_t tp_index; /* the position of dist_th_tp in dist_thr: the threshold whose matches give the true-positive errors */
} md_nusc_eval_attrs;
/* The greedy matching of the devkit's accumulate() for every (sample, class) cell and all D thresholds; one wave per cell, the ground
 * truths over the lanes in chunks of 64, the detections in row order (the walking order), the distance computed once per pair, one
 * taken-bit set per threshold, the winner from a wave reduction on (distance, ground-truth row).
 * in : gt_beg[C], gt_cnt[C], dt_beg[C], dt_cnt[C] i32 (C = I Kc), gt_xy[Gt,2], gt_size[Gt,3], gt_yaw[Gt], gt_vel[Gt,2] f64, gt_attr[Gt] i32,
 *      dt_xyz[Dt,3], dt_size[Dt,3], dt_yaw[Dt], dt_vel[Dt,2] f64, dt_attr[Dt] i32, dist_thr[D] f64, period[Kc] f64
 * out: dtm[D,Dt] i32 (the packed ground-truth row matched, -1 if none), err[Dt,5] f64 (trans, scale, orient, vel, attr of the match at
 *      threshold tp_index, zeros where unmatched), cell_ngt[C] i32.  Every element is written on every call.
 * extra: md_nusc_eval_attrs, required.
 * Per detection and threshold: among the cell's ground truths not yet taken at this threshold the smallest dist = sqrt(dx dx + dy dy) of
 * the xy centres wins, the lowest row on equal distance (a NaN or infinite distance never wins); it is a match if dist < dist_thr.  Then
 * trans = dist; scale = 1 - inter / ((va + vb) - inter) with v = (s0 s1) s2 and inter the same product of the smaller sizes; orient =
 * |angle_diff(gt_yaw, dt_yaw, period[k])| with d = pymod((x - y) + period / 2, period) - period / 2, minus 2 pi if d > pi, pymod = fmod
 * moved into [0, period); vel = sqrt(dvx dvx + dvy dvy) of gt - dt; attr = NaN if gt_attr < 0, else 1 - (gt_attr == dt_attr).
 * 2: an extent other than documented (C not a multiple of Kc), tp_index outside [0, D), aliasing.  4: C >= MD_NUSCEVAL_MAX_CELLS, Gt or
 * Dt > MD_NUSCEVAL_MAX_ROWS, D > MD_NUSCEVAL_MAX_THRS, Kc > MD_NUSCEVAL_MAX_CLASSES. */
int md_nusc_eval_match(MD_AOT_ARGS);

/* The curves of the devkit's accumulate(): one workgroup per (class, threshold).
 * in : order[Dt] i32 (detection rows, class-major; within a class in walking order across the samples: descending score, on equal
 *      scores the later sample first, inside a sample in row order), cat_off[Kc+1] i32 (class k owns order[cat_off[k] .. cat_off[k+1])),
 *      dt_score[Dt] f64, dtm[D,Dt] i32, err[Dt,5] f64, cell_ngt[C] i32 (C = I Kc), rec_thr[R] f64 (ascending)
 * out: precision[Kc,D,R], confidence[Kc,D,R], tp_err[Kc,5,R] f64, n_gt[Kc] i32 (the sum of cell_ngt over the samples), n_match[Kc,D] i32,
 *      and the named intermediates, indexed by the position in `order`: tp_scan[D,Dt] i32 (the running count of matches), m_conf[Dt] f64
 *      and m_cum[5,Dt] f64 (class k's matches at tp_index, compacted to cat_off[k] ..: their scores and the running means of their
 *      errors).  Every element is written on every call; positions outside a list are 0.
 * extra: md_nusc_eval_attrs, required.
 * Per (k, d): tp = the inclusive integer scan of dtm >= 0 over the class's list, fp = (j + 1) - tp; prec = tp / (fp + tp), rec = tp / n_gt;
 * precision = interp(rec_thr, rec, prec, right = 0), confidence = interp(rec_thr, rec, score, right = 0).  At d = tp_index, per metric:
 * the running sum is a serial chain in list order with NaN counted as 0 (np.cumsum's bits; one lane per metric, the values staged
 * through LDS), cm = sum / count of non-NaN, 0 while that count is 0, all ones if every value is NaN; tp_err = interp(confidence,
 * m_conf reversed, cm reversed), element by element.  n_gt == 0 or no match: precision and confidence 0, tp_err 1.
 * interp(x, xp, fp): j = the largest index with xp[j] <= x (binary search); x < xp[0]: fp[0]; x > xp[last]: right, or fp[last] without
 * one; x == xp[j] or j last: fp[j]; else s = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]), v = s (x - xp[j]) + fp[j]; if v is NaN,
 * v = s (x - xp[j+1]) + fp[j+1]; if still NaN and fp[j] == fp[j+1], fp[j].
 * 2: an extent other than documented (C not a multiple of Kc), tp_index outside [0, D), aliasing.  4: Kc > MD_NUSCEVAL_MAX_CLASSES,
 * C >= MD_NUSCEVAL_MAX_CELLS, Dt > MD_NUSCEVAL_MAX_ROWS, D > MD_NUSCEVAL_MAX_THRS, R > MD_NUSCEVAL_MAX_RECS. */
int md_nusc_eval_accumulate(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_NUSCEVAL_H_ */
