/*
 * minddet_hip_ppreader.h -- C ABI of the front end of the anchor-based (KITTI) PointPillars of libminddet_hip.so: its pillar feature
 * net with the scatter, and the anchor mask of a whole batch.  With md_voxelize (minddet_hip_points.h) in front they take the model
 * from raw points to the operands of the reference's own call, PointPillarsNet.construct(voxels, num_points, coors, anchors,
 * anchors_mask) (minddet/models/pointpillars/src/pointpillars.py:728-739), with nothing read back to the host.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions"), which this header includes.
 */
#ifndef MINDDET_HIP_PPREADER_H_
#define MINDDET_HIP_PPREADER_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_pp_pillar_encode_attrs {
    float vx, vy, vz;                   /* voxel_size x, y, z (pointpillars.py:264-266) */
    float x_offset, y_offset, z_offset; /* vx / 2 + pc_range[0], vy / 2 + pc_range[1], vz / 2 + pc_range[2] (:267-269) */
    int32_t with_distance;              /* 0: K = 10 features; 1: K = 11, the point's distance from the origin last (:305-307) */
    int32_t reserved0;                  /* must be 0 */
} md_pp_pillar_encode_attrs;
/* PillarFeatureNet + PointPillarsScatter of the KITTI model in one launch (plus the zero fill of the canvas):
 * minddet/models/pointpillars/src/pointpillars.py:180-364, inference, use_norm=True, one PFN layer (num_filters = (64,)).
 * in : voxels[B,MV,MP,4] f32, num_points[B,MV] i32, coors[B,MV,4] i32 (b, z, y, x), voxel_num[B] i32 (md_voxelize's outputs),
 *      w[64,K] f32: the RAW Dense weight (K = 10, or 11 with_distance), scale[64] f32, shift[64] f32: the BatchNorm (eps 1e-3, moving
 *      statistics) as scale = gamma / sqrt(var + 1e-3), shift = beta - mean * scale, folded in fp32 on the host.  The BatchNorm is NOT
 *      folded into w: the reference rounds the raw weight to fp16 (:197-200), so a folded weight would round differently.
 * out: canvas[B,H,W,64] bf16, NHWC (the reference scatters to [B,H,W,2,64] and transposes to NCHW, :349-362).
 * extra: md_pp_pillar_encode_attrs, required.
 * Per voxel row v < voxel_num[b], with n = clamp(num_points, 0, MP):
 *   mean  = (fp32 sum of the n points' xyz in row order) / max(n, 1): one correctly rounded fp32 divide (:279-282)
 *   f[r]  = [x, y, z, r, x - mean.x, y - mean.y, z - mean.z, x - (coors.x * vx + x_offset), y - (coors.y * vy + y_offset),
 *            z - (coors.z * vz + z_offset) (, dist)] for r < n (:282-308).  Every operation is ONE fp32 rounding, nothing is contracted
 *           into an FMA; dist = sqrt((x * x + y * y) + z * z), every operation rounded, the square root correctly rounded.  The tenth
 *           feature, the z offset from the pillar centre (:291-294), is what md_pillar_encode does not have.
 *           Rows n <= r < MP are zero (the padding mask, :311-314).
 *   Dense under to_float(float16) (:197-200): d[r][c] = fp16(sum_k fp16(w[c][k]) * fp16(f[r][k])).  Both operands are rounded to fp16
 *           with round-to-nearest-even; the products (exact in fp32) and their sum are in fp32, in any order; the result is rounded
 *           to fp16.
 *   BatchNorm on the fp16 tensor: y[r][c] = fp16(scale[c] * d[r][c] + shift[c]), computed in fp32 (an FMA or two roundings: either)
 *           and rounded to fp16; then ReLU.  MindSpore's BatchNorm arithmetic on an fp16 input is not part of the reference's
 *           sources: this form is the documented choice of this library, and parity with the framework is unpinned.
 *   m[c]  = max of y[r][c] over ALL MP rows (:218).  A padded row gives relu(fp16(shift[c])) and takes part in the maximum as in the
 *           reference; so a live row with n <= 0 gives relu(fp16(shift)), not zero: this model has no voxel mask, unlike
 *           CenterPoint's reader (md_pillar_encode).
 *   canvas[coors.b, coors.y, coors.x, :] = bf16(m), round to nearest even.
 * Rows >= voxel_num[b] and rows whose coors lie outside the canvas write nothing; other cells are zero.  Two rows with the same coors:
 * one of them wins.  Deterministic.  A non-finite input gives an unspecified value in its own cell only.
 * 2: F != 4, K not 10 / 11 or not the K of with_distance, mismatched shapes, a non-finite attribute or a voxel size <= 0,
 *    reserved0 != 0.   4: MP > 32 (the reference's configs use 32), extents whose element counts do not fit 32 bits. */
int md_pp_pillar_encode(MD_AOT_ARGS);

/* The anchor mask of pointpillars/src/data/preprocess.py:211-225 + core/box_np_ops.py:745-776 for a whole batch, with the number of
 * voxels of each sample read on the device.
 * in : coors[B,MV,4] i32 (b, z, y, x), voxel_num[B] i32 (md_voxelize's outputs), anchors_bv[N,4] f32
 * out: mask[B,N] u8 [, area[B,N] f32 or NULL] [, workspace u8: md_pp_anchor_mask_workspace_bytes(B, grid_x, grid_y) bytes, at
 *      least B * grid_y * grid_x * 4]
 * extra: md_anchor_mask_attrs (minddet_hip.h), required.
 * Row b equals, bit for bit, what md_anchor_mask gives for coors[b, :clamp(voxel_num[b], 0, MV), 1:] (both entries are in
 * csrc/ppreader.hip and launch one set of kernels, md_anchor_mask with B = 1 and every row counted): the voxels are counted per
 * (y, x) cell -- a voxel whose y or x is outside the grid is not counted, its b and z are not looked at -- then area = the count
 * inside the anchor's cell range from the integral image (integers: exact), mask = area > area_threshold.
 * 2: coors not [B,MV,4], voxel_num not [B], anchors_bv not [N,4], mask / area not [B,N].   4: grid_x or grid_y < 1, B x cells > 2^28,
 *    B x N or B x MV >= 2^31. */
int md_pp_anchor_mask(MD_AOT_ARGS);
int64_t md_pp_anchor_mask_workspace_bytes(int64_t B, int64_t grid_x, int64_t grid_y);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_PPREADER_H_ */
