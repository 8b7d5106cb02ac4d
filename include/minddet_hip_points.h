/*
 * minddet_hip_points.h -- C ABI of the point-cloud front end of libminddet_hip.so: the voxeliser and the fused pillar encoder.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions"), which this header includes.
 */
#ifndef MINDDET_HIP_POINTS_H_
#define MINDDET_HIP_POINTS_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_voxelize_attrs {
    float voxel_size[3]; /* x, y, z */
    float range[6];      /* x, y, z min, then x, y, z max */
    int32_t max_points;  /* == voxels.shape[2] */
    int32_t max_voxels;  /* == voxels.shape[1]; per sample */
} md_voxelize_attrs;
/* Device twin of points_to_voxel(reverse_index=True): minddet/models/centerpoint/det3d_ms/ops/point_cloud/point_cloud_ops.py:5-53,
 * 108-177 (minddet/models/pointpillars/src/core/point_cloud/point_cloud_ops.py is the same routine), for B samples in one call.
 * in : points[N,F] f32, F = 4 or 5 (x, y, z first), the B samples back to back; offsets[B+1] i32 (sample b = points
 *      [offsets[b], offsets[b+1]); device memory, non-decreasing, within [0, N])
 * out: voxels[B,max_voxels,max_points,F] f32, coors[B,max_voxels,4] i32 = (b, z, y, x), num_points[B,max_voxels] i32,
 *      voxel_num[B] i32 [, workspace u8: md_voxelize_workspace_bytes(N, B, gx gy gz, max_voxels) bytes; never more than
 *      4 * (2 B gx gy gz + 3 N + 2 B max_voxels + (N + B max_voxels) / 1024) + 4096].
 * extra: md_voxelize_attrs, required.  The grid is nearbyint((max - min) / voxel_size) cells per axis, computed in fp32 (:24-27).
 * The result equals the reference's sequential loop bit for bit: a point's cell is floor((p - min) / voxel_size) per axis with an
 * fp32 subtract and a correctly rounded fp32 divide; the point is dropped if any axis is outside [0, grid); voxels are numbered in the
 * order of their first point; a cell whose first point comes when max_voxels voxels exist is dropped with all its points; a voxel
 * keeps its first max_points points by index, in index order; unused rows and slots are zero.  voxel_num[b] is the number of voxels
 * of sample b (the reference returns max_voxels rows and leaves the count to the caller).  A point with a NaN or infinite x, y or z
 * is dropped; the reference is undefined there (it casts the NaN to an index).  Deterministic.
 * 2: F not 4 or 5, output shapes that do not match each other or the attributes, voxel_size <= 0, max <= min, a non-finite attribute.
 * 4: N, B x cells or B x max_voxels >= 2^30, B > 4096, max_points > 65536. */
int md_voxelize(MD_AOT_ARGS);
int64_t md_voxelize_workspace_bytes(int64_t N, int64_t B, int64_t cells, int64_t max_voxels);

typedef struct md_pillar_encode_attrs {
    float vx, vy;             /* voxel_size x, y (pillar_encoder.py:123-124) */
    float x_offset, y_offset; /* vx / 2 + pc_range[0], vy / 2 + pc_range[1] (:125-126) */
    int32_t with_distance;    /* must be 0 (:182-184 is not built) */
    int32_t virtual_points;   /* must be 0 (:138-143 is not built) */
} md_pillar_encode_attrs;
/* PillarFeatureNet + PointPillarsScatter in one launch (plus the zero fill of the canvas):
 * minddet/models/centerpoint/det3d_ms/models/readers/pillar_encoder.py:18-67,131-199,219-228, inference.
 * in : voxels[B,MV,MP,F] f32, num_points[B,MV] i32, coors[B,MV,4] i32 (b, z, y, x), voxel_num[B] i32 (md_voxelize's outputs),
 *      w1[C1,F+5] f32, b1[C1] f32, w2[64,64] f32 or NULL, b2[64] f32 or NULL: the PFN layers' Dense weights with the BatchNorm
 *      (eps 1e-3, moving statistics) folded in: w = weight * gamma / sqrt(var + eps) per output row, b = beta - mean * gamma /
 *      sqrt(var + eps).  One layer (num_filters = (64,)): C1 = 64, w2 = b2 = NULL.  Two layers ((64, 64)): C1 = 32 (:32-33).
 * out: canvas[B,H,W,64] bf16, NHWC (the reference scatters to NHWC and transposes to NCHW, :220-227).
 * extra: md_pillar_encode_attrs, required.
 * Per voxel row v < voxel_num[b] with n = min(num_points, MP) > 0 points, in fp32 with fp32 accumulation:
 *   mean  = (sum of the n points' xyz in row order) / n
 *   f[r]  = [point (F), xyz - mean (3), x - (coors.x * vx + x_offset), y - (coors.y * vy + y_offset)] for r < n, zero rows for
 *           r >= n (the padding mask, :189-193)
 *   layer : y[r] = relu(w f[r] + b); m = max over ALL MP rows -- a padded row gives relu(b), so for n < MP the maximum includes
 *           relu(b) (the reference does, :61); last layer: the output is m; otherwise the next input is [y[r], m] (:65-66), and the
 *           padded rows' next input is [relu(b1), m]
 *   canvas[coors.b, coors.y, coors.x, :] = bf16(m of the last layer), round to nearest even: the only bf16 rounding.
 * n <= 0: the voxel mask (:158, custom_bn.py:121) gives zeros.  Rows >= voxel_num[b] and rows whose coors lie outside the canvas
 * write nothing; cells without a pillar are zero.  Two rows with the same coors: one of them wins (the reference adds them).
 * 2: F not 4 or 5, widths other than the above, with_distance / virtual_points set, mismatched shapes.  4: MP > 64, extents
 * whose element counts do not fit 32 bits. */
int md_pillar_encode(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_POINTS_H_ */
