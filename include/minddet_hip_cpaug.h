/*
 * minddet_hip_cpaug.h -- C ABI of the CenterPoint (nuScenes) training input of libminddet_hip.so: the training branch of the Preprocess
 * step and the ground-truth filter of the Voxelization step (centerpoint/det3d_ms/datasets/pipelines/preprocess.py:46-157, 187-193)
 * between the raw points and the voxeliser: points_count_rbbox + the min_points_in_gt mask (:74-79, core/bbox/box_np_ops.py:9-14),
 * the accept step of the ground-truth sampler (core/sampler/sample_ops.py:127-154, 245-291), the point side of its result (:168-185)
 * and np.concatenate([sampled_points, points]), random_flip_both, global_rotation, global_scaling_v2, global_translate_
 * (core/sampler/preprocess.py:665-721, 812-834) and filter_gt_box_outside_range (:102-116), which the reference runs on the host.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 *
 * As in minddet_hip_pcaug.h: the ops contain no random number generator (every draw is a float64 operand), no floating-point atomics,
 * no memset, no host read; two calls give the same bits.  No output may share its address with an input or with another output: such a
 * call is refused with rc 2.  Every decision (a point inside a box, two boxes colliding, a corner inside the range) and every transform
 * is evaluated in float64 from the fp32 inputs and the float64 draws, and a value is rounded once, where an fp32 output is stored;
 * tests/cpaug_contract.py states the ops in numpy float64 together with the margin of every decision.
 *
 * A box is [x, y, z, w, l, h, vx, vy, r] in fp32.  global[B,7] f64 = (flip_a, flip_b, rot, scale, tx, ty, tz):
 *   flip_a (random_flip_both's first draw, its "x flip"): y -> -y, vy -> -vy, r -> -r + pi
 *   flip_b (its second draw, its "y flip"):               x -> -x, vx -> -vx, r -> -r + 2 pi   (the reference's "+ 2 pi", kept)
 *   rot: (x, y) -> (x cos + y sin, -x sin + y cos), the same for (vx, vy), r += rot; scale: columns 0-7 of a box (the velocities
 *   included, gt_boxes[:, :-1]), columns 0-2 of a point; (tx, ty, tz) added to columns 0-2.
 *
 * Reference quirks
 *  (a) box_collision_test: quirk (a) of minddet_hip_pcaug.h, the same predicate (csrc/aug_geom.h).
 *  (b) global_translate_ draws z with std[0] (:825-827): that belongs to the caller's draw, not to the ops.
 *  (c) sample_class_v2 forms the collision matrix once per call and resolves it in candidate order: a candidate is rejected by a later
 *      candidate of its call that has not been visited yet; in a chain c0-c1-c2 in which only neighbours collide c0 and c1 go and c2
 *      stays; a candidate that collides only with a rejected candidate of an earlier call, or with a ground-truth row that the
 *      min-points mask dropped, is accepted.  Kept.
 *  (d) scene points inside a sampled box are not removed.  Kept.
 *  (e) the avoid list holds the ground-truth rows of every name (the class mask comes later, :114): kept -- md_cp_aug_select reads
 *      `keep`, not the classes.
 * Not built (the Python layer refuses them with ValueError; the ABI has no operand for them): shuffle_points, flip_coor, group
 * sampling, the sampler's per-object global rotation (global_random_rotation_range_per_object other than [0, 0]), random_crop.
 */
#ifndef MINDDET_HIP_CPAUG_H_
#define MINDDET_HIP_CPAUG_H_

#include "minddet_hip_points.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_CPAUG_MAX_GT 512   /* G: ground-truth rows per sample (max_objs is 500 in the nuScenes config) */
#define MD_CPAUG_MAX_CAND 256 /* S: sampler candidates per sample */
#define MD_CPAUG_MAX_BATCH 4096

typedef struct md_cp_count_attrs {
    int32_t min_points; /* min_points_in_gt; <= 0: the mask keeps every row below gt_count */
} md_cp_count_attrs;
/* points_count_rbbox (box_np_ops.py:9-14, origin 0.5: the box frame is centred in z) and the min_points_in_gt mask (:74-79).
 * in : points[N,F] f32, F = 5 (the B samples back to back); offsets[B+1] i32 (as md_voxelize takes them); gt_boxes[B,G,9] f32;
 *      gt_count[B] i32 (a count outside [0, G] is clamped)
 * out: counts[B,G] i32 (0 for g >= gt_count[b]); keep[B,G] u8 = g < gt_count[b] and (min_points <= 0 or counts >= min_points) ;
 *      [workspace u8: md_cp_aug_count_points_workspace_bytes(B, G) bytes; never more than 96 B G; without it the library's per-stream
 *      scratch pool serves]
 * extra: md_cp_count_attrs, required.
 * Inside: with (dx, dy, dz) = p - (x, y, z) and (lx, ly) = (dx cos r - dy sin r, dx sin r + dy cos r): |lx| < w / 2, |ly| < l / 2 and
 * |dz| < h / 2, all strict.  A point before offsets[0] or from offsets[B] on belongs to no sample.
 * 2: F != 5, an extent other than documented.  4: N >= 2^30, G > MD_CPAUG_MAX_GT, B > MD_CPAUG_MAX_BATCH, a workspace smaller than
 * documented. */
int md_cp_aug_count_points(MD_AOT_ARGS);
int64_t md_cp_aug_count_points_workspace_bytes(int64_t B, int64_t G);

/* The accept step of sample_class_v2 (sample_ops.py:245-291) as sample_all drives it (:127-154), enable_global_rot false.
 * in : gt_boxes[B,G,9] f32, gt_count[B] i32, keep[B,G] u8 (md_cp_aug_count_points'), cand_boxes[B,S,9] f32 (the drawn database boxes
 *      in draw order), cand_count[B] i32 (clamped to [0, S]), cand_group[B,S] i32 (non-decreasing per sample; one value stands for
 *      one sample_class_v2 call)
 * out: accept[B,S] u8 (0 for s >= cand_count[b]) ; [workspace u8: md_cp_aug_select_workspace_bytes(B, G, S) bytes; never more
 *      than 8 B S ((G + S + 63) / 64); else the pool]
 * For each group in order: the matrix of box_collision_test over the avoid list (the kept ground-truth rows, then the candidates
 * accepted in earlier groups) followed by the group's candidates, the diagonal cleared; the group's candidates are walked in order: a
 * candidate whose row has a live column is rejected and its row and column are cleared, any other is accepted (quirk (c)).  BEV
 * corners: center_to_corner_box2d(xy, wl, r).  A sample whose cand_group decreases somewhere below cand_count is an argument error that
 * only the device can see: every candidate of that sample is rejected (accept 0), nothing is read back.
 * 2: an extent other than documented.  4: G > MD_CPAUG_MAX_GT, S > MD_CPAUG_MAX_CAND, B > MD_CPAUG_MAX_BATCH, a workspace smaller than
 * documented. */
int md_cp_aug_select(MD_AOT_ARGS);
int64_t md_cp_aug_select_workspace_bytes(int64_t B, int64_t G, int64_t S);

/* The point side of sample_all's result (:168-185, without rot_transform), np.concatenate([sampled_points, points]) and the point
 * side of the four global steps, as one stable compaction.
 * in : points[N,F] f32, F = 5; offsets[B+1] i32; cand_points[Ns,F] f32 (every candidate's points in its own frame, as the database file
 *      holds them, candidate after candidate), cand_offsets[B S + 1] i32, cand_boxes[B,S,9] f32, accept[B,S] u8 -- NULL all four or
 *      none (then Ns = 0); global[B,7] f64
 * out: points_out[N+Ns,F] f32, offsets_out[B+1] i32 ; [workspace u8: md_cp_aug_points_workspace_bytes(N, Ns, B) bytes; never more than
 *      64 B + (N + Ns) + 4 ((N + Ns) / 256 + 3); else the pool]
 * Per sample the output holds the accepted candidates' points in candidate order, each plus its box centre (x, y, z), then the scene
 * points in their order; then flip_a, flip_b, the rotation, the scale and the translation on columns 0-2.  Columns 3 and up pass
 * through bit for bit.  The samples sit back to back, zero rows behind the last kept row.
 * 2: F != 5, an extent other than documented, candidate operands given in part.  4: N + Ns >= 2^30, S > MD_CPAUG_MAX_CAND,
 * B > MD_CPAUG_MAX_BATCH, a workspace smaller than documented. */
int md_cp_aug_points(MD_AOT_ARGS);
int64_t md_cp_aug_points_workspace_bytes(int64_t N, int64_t Ns, int64_t B);

typedef struct md_cp_boxes_attrs {
    float bv_range[4]; /* x min, y min, x max, y max of the training range; finite */
} md_cp_boxes_attrs;
/* The gt_boxes_mask selection (:81-83, 114), the box side of the four global steps and filter_gt_box_outside_range (:187-191).
 * in : gt_boxes[B,G,9] f32, gt_classes[B,G] i32 (the global 1-based class, 0 for a name outside class_names), gt_count[B] i32,
 *      keep[B,G] u8; cand_boxes[B,S,9] f32, cand_classes[B,S] i32, accept[B,S] u8 -- NULL all three or none (then S = 0);
 *      global[B,7] f64
 * out: boxes_out[B,G+S,9] f32, classes_out[B,G+S] i32, out_count[B] i32
 * extra: md_cp_boxes_attrs, required.
 * Selected: the ground-truth rows with g < gt_count[b], keep set and class > 0, then the accepted candidates with class > 0.  Per
 * selected row: the two flips; (x, y) and (vx, vy) rotated, r += rot; columns 0-7 scaled; columns 0-2 translated; the row survives
 * if any BEV corner of (x, y, w, l, r) is strictly inside bv_range.  The survivors are compacted to the front in order; the rest is
 * zeros with class 0 (md_cp_assign_targets reads those as padding rows).  No limit_period: AssignLabel has its own.
 * 2: an extent other than documented, candidate operands given in part, a non-finite attribute.  4: G > MD_CPAUG_MAX_GT,
 * S > MD_CPAUG_MAX_CAND, B > MD_CPAUG_MAX_BATCH. */
int md_cp_aug_boxes(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_CPAUG_H_ */
