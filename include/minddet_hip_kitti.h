/*
 * minddet_hip_kitti.h -- C ABI of the two camera-frame ends of the KITTI PointPillars path of libminddet_hip.so: the cut of a raw
 * velodyne scan to the camera's view in front of md_voxelize / md_pc_augment_points, the label boxes from the camera frame into the
 * lidar frame, and the KITTI result rows behind md_pp_decode_selected.  What it replaces, all host numpy / numba in the reference:
 * remove_outside_points (pointpillars/src/core/box_np_ops.py:625-636, called from src/data/preprocess.py:69-71 and create_data.py:35),
 * the reference_detections lines of prep_pointcloud (src/data/preprocess.py:59-67), box_camera_to_lidar (box_np_ops.py:599-613, called
 * at src/data/preprocess.py:87), and generate_single_sample_dict_old + predict_kitti_to_anno (src/predict.py:204-262, 331-396).
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 *
 * As in minddet_hip_pcaug.h: no random number generator, no floating-point atomics, no memset, no host read; two calls give the same
 * bits.  No output may share its address with an input or with another output: such a call is refused with rc 2.  Every decision and
 * transform is evaluated in float64 from the fp32 inputs and the float64 matrices, products and sums from the left without
 * contraction, and a value is rounded once, where an fp32 output is stored; tests/kitti_io_contract.py states the three operators in
 * numpy float64 together with the margin of every decision.
 *
 * Calibration products are composed by the caller on the host in float64 and arrive as operands (det_ops.KittiCalibration): the
 * frustum corners, rect @ Trv2c and its inverse.  No QR factorisation and no matrix inverse runs on the device.
 *
 * Reference quirks
 *  (a) the image box divides u and v by the corner's camera Z, not by the third row of P2 @ [X, Y, Z, 1] (box_ops.py:641-668): kept.
 *  (b) prep_pointcloud calls remove_environment on boxes that are still in the camera frame (src/data/preprocess.py:79 runs before
 *      :87 converts them): not built, see below.
 *  (c) the reference evaluates these routines in the calibration arrays' dtype (fp32 in its info files): not kept, float64 here.
 * Not built (the Python layer refuses them with ValueError): remove_environment, random_crop, generate_single_sample_dict (the
 * use_self_train == False branch of predict.py), points that are not 4 wide, fp32-calibration arithmetic.
 */
#ifndef MINDDET_HIP_KITTI_H_
#define MINDDET_HIP_KITTI_H_

#include "minddet_hip_points.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_CROP_MAX_HULLS 64    /* K: hulls per sample (one image frustum, or one frustum per reference detection) */
#define MD_CROP_MAX_BATCH 4096  /* B of md_pc_crop_hulls */
#define MD_KITTI_MAX_DETS 512   /* M of md_kitti_rows (nms_post_max_size is 300 in the reference's configs) */
#define MD_KITTI_MAX_LABELS 4096 /* G of md_kitti_boxes_to_lidar */
#define MD_KITTI_MAX_BATCH 4096 /* B of md_kitti_boxes_to_lidar and md_kitti_rows */

/* points_in_convex_polygon_3d_jit (geometry.py:18-55) over corner_to_surfaces_3d_jit (box_np_ops.py:723-742) of a sample's convex
 * hexahedra, any(-1) over the hulls, and the selection points[mask] -- as a stable compaction.
 * in : points[N,4] f32, the B samples back to back; offsets[B+1] i32 (as md_voxelize takes them);
 *      hulls[B,K,8,3] f64: corners in the lidar frame, in the corner order of the reference's corner functions (get_frustum: the
 *      near rectangle, then the far one); hull_count[B] i32, clamped to [0, K]
 * out: points_out[N,4] f32 (each sample's kept points in their order, the samples back to back, zero rows behind the last kept point),
 *      offsets_out[B+1] i32, keep[N] u8 indexed like the input (1 kept; 0 dropped, or a point before offsets[0] or from offsets[B] on,
 *      which belongs to no sample) ; [workspace u8: md_pc_crop_hulls_workspace_bytes(N, B, K) bytes, never more than the
 *      192 B K + 4 (N / 256 + 3) bytes that always suffice; without it the library's per-stream scratch pool serves]
 * Planes: surface j of a hull takes the corners 0 1 2 3 / 7 6 5 4 / 0 3 7 4 / 1 5 6 2 / 0 4 5 1 / 3 2 6 7; from its first three
 * corners s0, s1, s2 (surface_equ_3d_jit, geometry.py:7-15): n = (s0 - s1) x (s1 - s2), d = -((n0 s0x + n1 s0y) + n2 s0z).
 * A point is outside a hull iff sign = ((px n0 + py n1) + pz n2) + d >= 0 for one of the six surfaces (geometry.py:46-54), so inside
 * means sign < 0 six times, strict; a NaN sign compares false as in the reference and puts the point outside of nothing.  A point is kept iff it is inside
 * at least one of the first hull_count[b] hulls; hull_count[b] == 0 keeps nothing (masks.any(-1) over zero columns).
 * Every kept value passes through bit for bit, column 3 included.
 * 2: an extent other than documented, F != 4, an output at the address of an input or of another output.  4: N >= 2^30,
 * K > MD_CROP_MAX_HULLS, B > MD_CROP_MAX_BATCH, a workspace smaller than documented. */
int md_pc_crop_hulls(MD_AOT_ARGS);
int64_t md_pc_crop_hulls_workspace_bytes(int64_t N, int64_t B, int64_t K);

/* box_camera_to_lidar (box_np_ops.py:599-613) for a batch of label rows.
 * in : boxes_cam[B,G,7] f32 (x, y, z, l, h, w, r in the rectified camera frame), gt_count[B] i32 (clamped to [0, G]),
 *      cam2lidar[B,4,4] f64, row-major: the host's inv(rect @ Trv2c)
 * out: boxes_lidar[B,G,7] f32 (x, y, z, w, l, h, r): xyz[i] = fp32(((m[i][0] x + m[i][1] y) + m[i][2] z) + m[i][3]); w, l, h and r
 *      are the input bits; the rows from the count on are zero.
 * 2: an extent other than documented, aliasing.  4: G > MD_KITTI_MAX_LABELS, B > MD_KITTI_MAX_BATCH. */
int md_kitti_boxes_to_lidar(MD_AOT_ARGS);

typedef struct md_kitti_rows_attrs {
    float limit_range[6]; /* post_center_limit_range: x, y, z min, x, y, z max of the lidar centre; read when use_limit; not NaN */
    int32_t use_limit;    /* 0 or 1 */
    int32_t lidar_input;  /* 0 or 1; 1 skips the image-box filter (predict.py:352) */
} md_kitti_rows_attrs;
/* generate_single_sample_dict_old without its direction flip (md_pp_decode_selected has applied it) + predict_kitti_to_anno.
 * in : dets[B,M,9] f32 (x, y, z, w, l, h, r, score, label) and count[B] i32 (clamped to [0, M]) as md_pp_decode_selected and
 *      md_pack_detections leave them; lidar2cam[B,4,4] f64 (rect @ Trv2c); p2[B,4,4] f64; image_shape[B,2] i32 (h, w)
 * out: rows[B,M,14] f32 = alpha, bbox x1 y1 x2 y2, dimensions l h w, location x y z, rotation_y, score, label; src[B,M] i32: the
 *      row's index in dets, -1 behind out_count[b]; out_count[B] i32.  The survivors are compacted to the front in order, the rest
 *      of rows is zero.
 * extra: md_kitti_rows_attrs, required.
 * Per detection: location = rows 0-2 of lidar2cam @ [x, y, z, 1]; the eight corners (xc, yc, zc) = (+-l/2, 0 / -h, +-w/2) in the
 * order of box_ops.py:550-631, each taken to (xc cos r + zc sin r, yc, -xc sin r + zc cos r) + location; u = (((p[0][0] X +
 * p[0][1] Y) + p[0][2] Z) + p[0][3]) / Z and v from row 1 alike (quirk (a)); bbox = min / max over the corners, a NaN staying a NaN as
 * numpy's min and max keep it.  Dropped if !lidar_input and (x1 > W or y1 > H or x2 < 0 or y2 < 0); dropped if use_limit and the lidar
 * centre is below limit_range[0:3] or above limit_range[3:6] in any coordinate (the fp32 limits widened to float64); a NaN compares
 * false everywhere, so such a row is kept.  Then x2 = W where W < x2, y2 = H where H < y2, x1 = 0 where 0 > x1, y1 = 0 where 0 > y1;
 * alpha = -atan2(-y_lidar, x_lidar) + r.  l, h, w, r, score and label are the input bits.
 * 2: an extent other than documented, use_limit or lidar_input not 0 / 1, a NaN limit with use_limit, aliasing.
 * 4: M > MD_KITTI_MAX_DETS, B > MD_KITTI_MAX_BATCH. */
int md_kitti_rows(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_KITTI_H_ */
