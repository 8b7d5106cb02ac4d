/*
 * minddet_hip_pcaug.h -- C ABI of the KITTI PointPillars training augmentation of libminddet_hip.so: the training branch of
 * prep_pointcloud (minddet/models/pointpillars/src/data/preprocess.py:124-170) between the raw points and the voxeliser:
 * remove_points_in_boxes, noise_per_object, random_flip, global_rotation, global_scaling, global_translate,
 * filter_gt_box_outside_range and limit_period (src/core/preprocess.py:155-160, 365-451, 560-807, src/core/geometry.py:6-96,
 * src/core/box_np_ops.py:126-170, 195-360, 390-392, 682-742), which the reference runs as numba loops on the host.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 *
 * The ops contain no random number generator: the caller passes every random draw as a float64 tensor, so each op is a deterministic
 * function of its operands.  No atomics, no memset, no host read; two calls give the same bits.  No output may share its address with
 * an input or with another output: such a call is refused with rc 2.
 *
 * Precision (a stated choice, as for the losses and md_cp_assign_targets): every decision (a point inside a box, two boxes
 * colliding, a corner inside the range) and every transform is evaluated in float64 from the fp32 inputs and the float64 draws, and a
 * value is rounded once, where an fp32 output is stored.  The reference works in the arrays' dtype (fp32 boxes and points, see quirk
 * (e)), so its results agree with these within a forward bound, not bit for bit; tests/pcaug_contract.py states the ops in numpy
 * float64 together with the margin of every decision.
 *
 * Reference quirks
 *  (a) box_collision_test (:730-745) reads `if ret[i, j] is False`: a value comparison under numba, never true for a numpy bool under
 *      an identity comparison, in which case the containment tests are skipped.  Built here is the text's evident meaning: inside the
 *      standup (axis-aligned bounds) pre-test, collision = two edges cross, or A covers every corner of B, or B covers every corner of A.
 *  (b) global_translate draws z with std[0] (:800): that belongs to the caller's draw, not to the ops.
 *  (c) the flip maps r to -r + pi (:693): kept.
 *  (d) flip, rotation, scaling and translation apply to every box before the range filter: kept.
 *  (e) the reference stores rot_mat_t in the points' dtype (fp32 sines and cosines): not kept, see Precision.
 * Not built (the Python layer refuses them with ValueError; the ABI has no operand for them): group_ids, boxes wider than 7,
 * reference_detections, remove_environment, remove_outside_points, without_reflectivity, bev_only, shuffle_points.
 */
#ifndef MINDDET_HIP_PCAUG_H_
#define MINDDET_HIP_PCAUG_H_

#include "minddet_hip_points.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_PCAUG_MAX_BOXES 256 /* per sample: G, and R of the remove boxes */
#define MD_PCAUG_MAX_TRIES 128 /* T */
#define MD_PCAUG_MAX_BATCH 4096

/* noise_per_object without groups (src/core/preprocess.py:560-668: noise_per_box :211-239, noise_per_box_v2_ :365-420,
 * _select_transform :454-460, box3d_transform_ :444-451) for B samples.
 * in : gt_boxes[B,G,7] f32 (lidar x, y, z, w, l, h, r), gt_count[B] i32, valid[B,G] u8 (the reference's gt_boxes_mask),
 *      loc_noises[B,G,T,3] f64, rot_noises[B,G,T] f64, grot_noises[B,G,T] f64 or NULL (NULL: noise_per_box, the enable_grot == False
 *      branch of :642-653)
 * out: selected[B,G] i32 (the first try whose box collides with no other box, or -1), obj_transform[B,G,4] f64 = (loc x, y, z, rot) of
 *      the selected try -- in the v2 form with the global-rotation displacement added as :417-418 add it in place -- zeros where
 *      selected is -1; boxes_out[B,G,7] f32 = the boxes after box3d_transform_.
 * Rows g >= gt_count[b] (a count outside [0, G] is clamped) take part in nothing: -1 and zeros.  A row that is not valid does not move
 * (selected -1, its box copied) but the other boxes collide with it (:386-387, 410-413).  Boxes are walked in index order and box i is
 * tested against the corners the earlier boxes ended up with (:416).  A try's corners: the box's (w, l) rectangle rotated by r (v2:
 * by r + the try's global rotation g, its centre turned about the origin by g -- the reference's radius sin / cos of atan2(x, y) + g,
 * formed as the displacement x (cos g - 1) + y sin g, y (cos g - 1) - x sin g, which is also what obj_transform's loc gains), rotated by the
 * try's rot about the centre, moved by the try's loc x, y.  Collision: quirk (a).
 * 2: an extent other than documented, T < 1.  4: G > MD_PCAUG_MAX_BOXES, T > MD_PCAUG_MAX_TRIES, B > MD_PCAUG_MAX_BATCH. */
int md_pc_noise_per_object(MD_AOT_ARGS);

/* remove_points_in_boxes (:155-159) + points_in_convex_polygon_3d_jit (geometry.py:18-55) on the boxes BEFORE the noise (the reference
 * takes the masks from gt_box_corners of :620) + points_transform_ (:423-441) + the point side of random_flip / global_rotation /
 * global_scaling / global_translate (:671-705, 788-807) + a stable compaction.
 * in : points[N,4] f32, the B samples back to back; offsets[B+1] i32 (as md_voxelize takes them); obj_boxes[B,G,7] f32 (before the
 *      noise), gt_count[B] i32, valid[B,G] u8, obj_transform[B,G,4] f64 (md_pc_noise_per_object's);
 *      remove_boxes[B,R,7] f32, remove_count[B] i32, remove_from[B] i32 -- NULL all three or none;
 *      global[B,6] f64 = (flip 0 / 1, rotation, scale, tx, ty, tz)
 * out: points_out[N,4] f32 (each sample's kept points in their order, the samples back to back, zero rows behind the last kept point),
 *      offsets_out[B+1] i32, owner[N] i32 indexed like the input (the first VALID box g < gt_count[b] that contains the point: only
 *      that box's transform is applied, :434-441; -1: none; -2: dropped) ; [workspace u8: md_pc_augment_points_workspace_bytes(N, B, G, R) bytes; never
 *      more than 128 B (G + R) + 64 B + 4 (N / 256 + 3); without it the library's per-stream scratch pool serves]
 * A point of sample b whose index within the sample is >= remove_from[b] and which lies in one of the first remove_count[b] remove
 * boxes is dropped (the points in front are the sampled objects' own, data/preprocess.py:124-127).  A point before offsets[0] or from
 * offsets[B] on belongs to no sample and is dropped.
 * Inside: with (dx, dy, dz) = p - (x, y, z) and (lx, ly) = (dx cos r - dy sin r, dx sin r + dy cos r): |lx| < w / 2, |ly| < l / 2 and
 * 0 < dz < h, all strict (the reference: sign >= 0 -> outside, geometry.py:46-54).
 * Per-object transform: subtract the centre, rotate about z by the transform's angle ((x, y) -> (x cos + y sin, -x sin + y cos)), add
 * the centre, add loc; a zero transform is the identity.  Then y = -y if flip, the global rotation (same sense), the scale, the
 * translation.  Column 3 passes through.
 * 2: F != 4, an extent other than documented, remove operands given in part.  4: N >= 2^30, G or R > MD_PCAUG_MAX_BOXES,
 * B > MD_PCAUG_MAX_BATCH, a workspace smaller than documented. */
int md_pc_augment_points(MD_AOT_ARGS);
int64_t md_pc_augment_points_workspace_bytes(int64_t N, int64_t B, int64_t G, int64_t R);

typedef struct md_pc_boxes_attrs {
    float bv_range[4]; /* x min, y min, x max, y max of the training range; finite */
} md_pc_boxes_attrs;
/* The box side of random_flip / global_rotation / global_scaling / global_translate (:671-705, 788-807), then
 * filter_gt_box_outside_range (:138-152), limit_period(r, 0.5, 2 pi) (box_np_ops.py:390-392) and the gt_boxes_mask selection of
 * data/preprocess.py:147-151.
 * in : boxes[B,G,7] f32 (md_pc_noise_per_object's boxes_out), gt_count[B] i32, valid[B,G] u8, classes[B,G] i32, global[B,6] f64
 * out: gt_boxes[B,G,7] f32, gt_classes[B,G] i32 (the rows with valid and any BEV corner strictly inside the range, compacted to the
 *      front in order; the rest zero), out_count[B] i32
 * extra: md_pc_boxes_attrs, required.
 * Per box: y = -y and r = -r + pi if flip (quirk (c)); (x, y) rotated, r += rotation; x, y, z, w, l, h scaled; x, y, z translated;
 * the four BEV corners (+-w / 2, +-l / 2) rotated by r about the centre; r = r - floor(r / (2 pi) + 0.5) 2 pi.
 * 2: an extent other than documented, a non-finite attribute.  4: G > MD_PCAUG_MAX_BOXES, B > MD_PCAUG_MAX_BATCH. */
int md_pc_augment_boxes(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_PCAUG_H_ */
