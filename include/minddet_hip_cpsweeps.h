/*
 * minddet_hip_cpsweeps.h -- C ABI of the CenterPoint (nuScenes) multi-sweep input of libminddet_hip.so: the step between a LiDAR
 * driver's buffers and md_voxelize / md_cp_aug_*.  What it replaces: read_sweep per past sweep and the concatenation of the nuScenes
 * branch of LoadPointCloudFromFile.__call__ (centerpoint/det3d_ms/datasets/pipelines/loading.py:56-80, 133-159), host numpy in the
 * reference's loader; its deployment demo does the same step on the GPU (tools_ms/multi_sweep_inference_ros.py:194-270).
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 *
 * As in minddet_hip_cpaug.h: no random number generator (the order of the sweeps is the caller's table), no floating-point atomics,
 * no memset, no host read; two calls give the same bits.  No output may share its address with an input or with another output: such
 * a call is refused with rc 2.  The keep decision is an fp32 comparison of the input values; the transform is evaluated in float64
 * from the fp32 inputs and the float64 matrix and rounded once, where the fp32 output is stored; tests/cp_sweeps_contract.py states
 * the operator in numpy float64.
 *
 * Reference quirks, kept (they are the caller's tables, the operator serves any of them)
 *  (a) the key frame is neither filtered nor transformed (loading.py:137-140): its flags are 0 and its time is 0.
 *  (b) the padding sweeps that nusc_common.py:443-450 adds when a scene has fewer past sweeps have transform_matrix None and time
 *      lag 0 but still pass through remove_close: flags 1.
 *  (c) the order of the past sweeps is np.random.choice(len(sweeps), nsweeps - 1, replace=False) (loading.py:148), a random
 *      permutation: the caller's draw, listed in seg_range.
 *  (d) the demo lists the sweeps oldest first with the current frame last and filters nothing (flags 2, the last 0): the same
 *      operator with another table.
 * Out of scope: shuffle_points (on the device a keyed sort, see det_ops.CenterPointAugment), the Waymo branch (tanh of the intensity,
 * elongation), `virtual` points, reading files, composing poses from quaternions on the device (the 4x4 arrives as 12 float64).
 */
#ifndef MINDDET_HIP_CPSWEEPS_H_
#define MINDDET_HIP_CPSWEEPS_H_

#include "minddet_hip_points.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_CPSWEEPS_MAX_SWEEPS 32 /* S: segments per sample (ten sweeps in the nuScenes configs) */
#define MD_CPSWEEPS_MAX_BATCH 256 /* B */

typedef struct md_cp_sweeps_attrs {
    float radius;      /* remove_close's radius (min_distance, 1.0 in read_sweep); finite, >= 0 */
    int32_t reserved0; /* must be 0 */
} md_cp_sweeps_attrs;
/* remove_close, the 4x4 transform into the key frame, the time column and the concatenation, as one stable compaction.
 * in : points[N,Fin] f32, Fin = 4 or 5: one pool of rows (a whole ring buffer, say); columns 0-3 (x, y, z, intensity) are read, a
 *      fifth column (the nuScenes ring index) is ignored as read_file does with [:, :4];
 *      seg_range[B,S,2] i32: (begin, end) row ranges into points, in output order per sample; end <= begin is an empty segment; the
 *      ranges may lie anywhere in [0, N] in any order (a ring needs no copy); together they hold at most N rows;
 *      transforms[B,S,12] f64: rows 0-2 of the 4x4, row-major; time_lag[B,S] f64;
 *      seg_flags[B,S] i32: bit 0 = apply remove_close, bit 1 = apply the transform; the other bits are reserved, 0, and not read
 * out: points_out[M,5] f32, M >= N; offsets_out[B+1] i32; status[B] i32 ;
 *      [workspace u8: md_cp_sweeps_merge_workspace_bytes(N, B, S) bytes, never more than the 4 (N / 256 + B S + 3) bytes that
 *      always suffice; without it the library's per-stream scratch pool serves]
 * extra: md_cp_sweeps_attrs, required.
 * Per sample, per segment in the listed order, per row in row order: with bit 0 the row is dropped if fabsf(x) < radius &&
 * fabsf(y) < radius on the untransformed fp32 values, both strict (a NaN coordinate compares false: the row is kept, as in numpy).
 * A kept row's xyz with bit 1: fp32(m[r][0] x + m[r][1] y + m[r][2] z + m[r][3]), the products and the sum from the left in float64
 * without contraction; with bit 1 clear: the input bits.  Column 3 passes through bit for bit; column 4 is fp32(time_lag).
 * The samples sit back to back: sample b is rows [offsets_out[b], offsets_out[b+1]), offsets_out[0] = 0; the rows from
 * offsets_out[B] to M are zeros, written by the operator.
 * Errors that only the device can see (nothing is read back):
 *   status[b] bit 0: a begin or an end of sample b lies outside [0, N]; that sample's output is empty
 *   status[b] bit 1, on every sample: the segments whose range lies in [0, N] hold more than N rows together; every sample is empty
 * 2: an extent or dtype other than documented, Fin not 4 or 5, M < N, reserved0 != 0, a negative or non-finite radius, an output at
 * the address of an input or of another output.  4: N or M >= 2^30, S > MD_CPSWEEPS_MAX_SWEEPS, B > MD_CPSWEEPS_MAX_BATCH, a
 * workspace smaller than documented. */
int md_cp_sweeps_merge(MD_AOT_ARGS);
int64_t md_cp_sweeps_merge_workspace_bytes(int64_t N, int64_t B, int64_t S);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_CPSWEEPS_H_ */
