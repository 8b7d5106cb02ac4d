/*
 * minddet_hip_cocoeval.h -- C ABI of the COCO bbox AP evaluation of libminddet_hip.so: from the fixed-shape output of a 2D detector
 * (dets [B, max_det, 6], count [B]) and packed ground truth to the precision [T, R, Kc, A, M] and recall [T, Kc, A, M] tables that
 * COCOeval.summarize() reads.  What it replaces, host Python in the reference: to_float / convert_eval_format
 * (centernet/src/post_process.py:64-89) and the COCOeval(coco, coco_dets, "bbox") evaluate() / accumulate() the reference calls at
 * centernet/eval.py:181-187.  minddet_amd/coco_eval.py states the same rules on the host (dets_to_coco, COCOBboxEval) and is the judge of
 * these operators; the twelve means of summarize() stay on the host, on the two tables.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 *
 * No random number generator, no floating-point atomics, no memset, no host read, no workspace and no use of the scratch pool: every
 * intermediate buffer is a named output operand sized from extents the host knows, and two calls give the same bits.  No output may
 * share its address with an input or with another output: such a call is refused with rc 2.  Every decision is evaluated in float64
 * from the operands without contraction, in the order coco_eval.py writes the operations; a value is rounded once, where it is stored.
 *
 * Packed layout (coco_eval.pack_coco).  I images in ascending image id, Kc categories in ascending id, cell c = i Kc + k; A area ranges
 * (4), T IoU thresholds (10), R recall thresholds (101), M maxDets values (3); Gt ground-truth rows, Dt detection rows.
 *   gt_beg, gt_cnt, dt_beg, dt_cnt [I Kc] i32: a cell owns the rows [beg, beg + cnt).  "Begin + count" so that a compact host packing and
 *     the padded per-image layout of md_coco_eval_rows both fit; rows outside every cell are never read.
 *   gt_box[Gt,4] f64 xywh, gt_area[Gt] f64, gt_crowd[Gt] u8, gt_ignore[Gt] u8 (ignore or iscrowd)
 *   dt_box[Dt,4] f64 xywh, dt_area[Dt] f64, dt_score[Dt] f64, dt_cat[Dt] i32 (k, or Kc for an unused row), dt_rank[Dt] i32 (the place
 *     inside the cell).  A cell's detection rows are in descending score order, equal scores in the order of the input records, and the
 *     cell is cut at MD_COCOEVAL_MAX_DETS rows, the last maxDets value.
 *   iou_thr[T], rec_thr[R], area_rng[A,2] f64: copied from COCOBboxEval's arrays so both sides compare against the same bits;
 *   max_dets[M] i32.
 *
 * Limits.  The host checks what the extents say (rc 4): the number of cells, Kc, Gt, Dt, max_det, T, A, R, M.  The per-cell counts are
 * device data: the kernels clamp them to the limit and skip a cell whose rows leave the operands (so nothing is read or written out
 * of bounds); the Python layer (coco_eval.pack_coco, det_ops) raises ValueError before any call.
 */
#ifndef MINDDET_HIP_COCOEVAL_H_
#define MINDDET_HIP_COCOEVAL_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_COCOEVAL_MAX_DETS 100        /* detections per cell: the last maxDets value */
#define MD_COCOEVAL_MAX_GTS 256         /* ground truths per cell */
#define MD_COCOEVAL_MAX_IMAGE_DETS 512  /* max_det: detection rows per image of md_coco_eval_rows */
#define MD_COCOEVAL_MAX_CELLS 16777216  /* I Kc stays below this (2^24) */
#define MD_COCOEVAL_MAX_CATS 128        /* Kc */
#define MD_COCOEVAL_MAX_ROWS 67108864   /* Gt, Dt (2^26) */
#define MD_COCOEVAL_MAX_LABELS 4096     /* L: entries of label_to_k */
#define MD_COCOEVAL_MAX_THRS 16         /* T */
#define MD_COCOEVAL_MAX_AREAS 8         /* A */
#define MD_COCOEVAL_MAX_RECS 256        /* R */
#define MD_COCOEVAL_MAX_MAXDETS 8       /* M */

typedef struct md_coco_eval_rows_attrs {
    int32_t first_image; /* the batch's first image: sample b writes the rows and cells of image first_image + b */
} md_coco_eval_rows_attrs;
/* dets_to_coco + the grouping into cells for one batch, nothing read back; one workgroup per image, rank by counting.
 * in : dets[B,max_det,6] f32 (x1, y1, x2, y2, score, label), count[B] i32, label_to_k[L] i32 (-1 drops the row)
 * out: dt_box[Dt,4] f64, dt_area[Dt] f64, dt_score[Dt] f64, dt_cat[Dt] i32, dt_rank[Dt] i32, dt_beg[I Kc] i32, dt_cnt[I Kc] i32,
 *      dt_src[Dt] i32 (the source row, -1 for an unused one); Dt = I max_det.  Image i owns the rows [i max_det, (i + 1) max_det) and
 *      the cells [i Kc, (i + 1) Kc); the call writes every element of the images first_image .. first_image + B - 1 and nothing else.
 * extra: md_coco_eval_rows_attrs, required.
 * Row r < min(count, max_det) is taken when its label l (truncated to an integer) lies in [0, L) and 0 <= label_to_k[l] < Kc.  Widened
 * to float64: x = to_float(x1), y = to_float(y1), w = to_float(x2 - x1), h = to_float(y2 - y1), score = to_float(score), area = w h,
 * with to_float(v) = float("{:.2f}".format(v)) done exactly: p = v 100, e = fma(v, 100, -p) (the exact error of p), n = rint(p),
 * f = p - n; n + 1 if f == 0.5 and e > 0; n - 1 if f == -0.5 and e < 0; n / 100.0.  The place of a row inside its image is its rank
 * under the key (k, -score after rounding, source row); rows beyond MD_COCOEVAL_MAX_DETS in a cell become unused.  Unused rows: box,
 * area and score 0, dt_cat Kc, dt_rank 0, dt_src -1.
 * 2: an extent other than documented (Dt not I max_det, cells not a multiple of I), first_image < 0 or first_image + B > I, aliasing.
 * 4: max_det > MD_COCOEVAL_MAX_IMAGE_DETS, L > MD_COCOEVAL_MAX_LABELS, Kc > MD_COCOEVAL_MAX_CATS, cells >= MD_COCOEVAL_MAX_CELLS,
 * Dt > MD_COCOEVAL_MAX_ROWS. */
int md_coco_eval_rows(MD_AOT_ARGS);

/* COCOBboxEval._evaluate_img for every (cell, area range) and all T thresholds; one wave per (cell, area range), the ground truths over
 * the lanes in chunks of 64, the detections in row order, the IoU computed on the fly.
 * in : gt_beg[C] i32, gt_cnt[C] i32, dt_beg[C] i32, dt_cnt[C] i32 (C = I Kc cells), gt_box[Gt,4] f64, gt_area[Gt] f64, gt_crowd[Gt] u8,
 *      gt_ignore[Gt] u8, dt_box[Dt,4] f64, dt_area[Dt] f64, iou_thr[T] f64, area_rng[A,2] f64
 * out: dtm[A,T,Dt] i32 (the packed ground-truth row matched, -1 if none), dt_ig[A,T,Dt] u8, cell_ngt[A,C] i32 (the counted ground
 *      truths of the cell).  Every element is written on every call; rows outside every cell are -1 / 0.
 * _iou_xywh of a pair: iw = min(dx + dw, gx + gw) - max(dx, gx) clipped at 0, ih alike, inter = iw ih, union = (da + ga) - inter with
 * da = dw dh and ga = gw gh, or da for a crowd ground truth; inter / union, 0 where union <= 0.
 * A ground truth is ignored when gt_ignore is set or gt_area < lo or gt_area > hi (both ends inclusive); it is available when no
 * detection holds it at this threshold, or when it is a crowd.  A candidate is available and has iou >= min(thr, 1 - 1e-10).  The winner
 * is the largest IoU among the counted candidates, the highest row on equal IoU; only if there is none, the same rule among the ignored
 * candidates.  dt_ig is the winner's ignore flag; for an unmatched detection it is dt_area < lo or dt_area > hi.
 * 2: an extent other than documented, aliasing.  4: C >= MD_COCOEVAL_MAX_CELLS, Gt or Dt > MD_COCOEVAL_MAX_ROWS,
 * T > MD_COCOEVAL_MAX_THRS, A > MD_COCOEVAL_MAX_AREAS, A T Dt >= 2^31. */
int md_coco_eval_match(MD_AOT_ARGS);

/* The body of COCOBboxEval.evaluate(): one workgroup per (k, a, m, t).
 * in : order[Dt] i32 (detection rows, category-major; within a category in descending score order, equal scores in row order: the
 *      host's (image, rank) order), cat_off[Kc+1] i32 (category k owns order[cat_off[k] .. cat_off[k+1])), dt_rank[Dt] i32,
 *      dtm[A,T,Dt] i32, dt_ig[A,T,Dt] u8, cell_ngt[A,C] i32 (C = I Kc), rec_thr[R] f64 (ascending), max_dets[M] i32
 * out: precision[T,R,Kc,A,M] f64, recall[T,Kc,A,M] f64, n_gt[A,Kc] i32 (the sum of cell_ngt over the images, an integer block sum)
 * Per (k, a, m, t): the subsequence of the category's list with dt_rank < max_dets[m]; tp and fp are the running counts of
 * matched-and-not-ignored and unmatched-and-not-ignored rows (integer scans); rc = tp / n_gt, pr = tp / ((fp + tp) + 2^-52); per recall
 * threshold q = the maximum of pr over the elements with rc >= thr (the envelope at searchsorted-left), 0 if there is none; recall is
 * the last rc, 0 for an empty list.  Both tables are -1 where n_gt == 0.  A maximum is exact in any order.
 * 2: an extent other than documented (C not a multiple of Kc), aliasing.  4: Kc > MD_COCOEVAL_MAX_CATS, C >= MD_COCOEVAL_MAX_CELLS,
 * Dt > MD_COCOEVAL_MAX_ROWS, T, A, R, M beyond their limits, A T Dt >= 2^31. */
int md_coco_eval_accumulate(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_COCOEVAL_H_ */
