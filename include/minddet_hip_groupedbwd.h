/*
 * minddet_hip_groupedbwd.h -- C ABI of the two operators of libminddet_hip.so that carry a gradient through md_conv2d_grouped
 * (include/minddet_hip.h), the one launch that runs the last conv of every SepHead branch of CenterPoint's CenterHead (csrc/convbwd.hip):
 * the data gradient of the grouped conv, optionally through the ReLU that made its input, and the weight and bias gradient of every group.
 * With md_conv_bwd_weight (minddet_hip_convbwd.h) for the merged first convs and md_adam_step (minddet_hip_train.h) CenterHead trains on the
 * device: md_cp_loss_grad -> md_conv2d_grouped_bwd_weight -> md_conv2d_grouped_bwd_data -> md_conv_bwd_weight (in dy_c_off chunks of at most
 * MD_CONV_BWD_MAX_COUT output channels) -> md_grad_sumsq -> md_adam_step, no host read, no floating-point atomic, no launch that waits on
 * another workgroup.
 * Both operators take the forward call's own table, md_conv2d_grouped_attrs, as `extra`: k, groups, cin_g = 64, x_c_off, cout[], y_off[],
 * w_row[]; relu must be 0 (the gradient of a ReLU behind the grouped conv is not built).
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 */
#ifndef MINDDET_HIP_GROUPEDBWD_H_
#define MINDDET_HIP_GROUPEDBWD_H_

#include "minddet_hip_convbwd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Input gradient of md_conv2d_grouped, optionally through the ReLU that made its input.  With q = (n, h, w) a pixel, tap t = k ky + kx and
 * its offset d_t = (ky - k / 2, kx - k / 2) rows and columns (the forward pass reads x[q + d_t] for y[q]):
 *   dx[q, x_c_off + 64 g + i] = sum_{t < k k} sum_{o < cout[g]} dy[q - d_t, y_off[g] + o] w[w_row[g] + o, t 64 + i]      (g < groups, i < 64)
 *   a term is zero where q - d_t leaves q's own image
 *   with act: dx = +0.0 unless act[q, x_c_off + 64 g + i] > 0       (a -0, a negative value or a NaN in act gives +0.0; the rule of
 *                                                                    md_conv1x1_bwd_data)
 * in : dy[N,H,W,Cy] f32 (the gradient w.r.t. the grouped conv's output), w[R, k k 64] bf16 (the grouped pack the forward pass read),
 *      act[N,H,W,Ca] bf16 or NULL (the ReLU's output: the tensor the forward pass read as x, at the same channels)
 * out: dx[N,H,W,Cdx] f32: channels [x_c_off, x_c_off + 64 groups) are written, every other channel is left as it was
 * extra: md_conv2d_grouped_attrs, required.
 * One launch, no workspace.  A workgroup owns MD_GROUPED_BWD_TILE consecutive pixels (of the flat index (n, h, w): a tile may span rows and
 * images, every lane tests its own tap against its own image) and walks MD_GROUPED_BWD_WALK groups; a wave takes 16 pixels as the rows of
 * the fp32 MFMA (v_mfma_f32_16x16x4_f32) with (t, o) as the reduction index, dy as it is (24 bits) and w widened to fp32 (exact).  Order of
 * the additions (fixed): one accumulator chain per element over (t, o) ascending, four o per MFMA (the MFMA is an fp32 fma chain, every
 * product rounded once into the accumulator; o is padded to a multiple of four with exact zeros).  The chain of roundings behind an element
 * is
 *   Ld(k, cout) = k k cout
 * and |dx - exact| <= Ld 2^-24 sum_{t, o} |dy w|.  The result is the same from call to call and from stream to stream.
 * 2: an extent other than documented, N, H or W < 1, k not 1 or 3, relu != 0, cin_g != 64, groups outside [1, MD_GROUPED_MAX_GROUPS],
 *    reserved0 != 0, x_c_off < 0 or x_c_off + 64 groups outside dx or act, a cout outside [1, 16], a y_off range outside dy, a w_row range
 *    outside w, w not [R, k k 64], dx at the address of another operand.
 * 4: P = N H W or an operand of 2^31 elements or more. */
#define MD_GROUPED_BWD_TILE 64
#define MD_GROUPED_BWD_WALK 4
int md_conv2d_grouped_bwd_data(MD_AOT_ARGS);

/* Weight and bias gradient of every group of md_conv2d_grouped in one pair of launches, in the grouped pack's layout:
 *   dw[w_row[g] + o, t 64 + i] = sum_p dy[p, y_off[g] + o] x[p + d_t, x_c_off + 64 g + i],   db[w_row[g] + o] = sum_p dy[p, y_off[g] + o]
 * (x = 0 where p + d_t leaves p's own image).
 * in : x[N,H,W,C] bf16 (group g reads channels [x_c_off + 64 g, + 64)), dy[N,H,W,Cy] f32
 * out: dw[R, k k 64] f32, db[R] f32 or NULL: every element is written, rows that no group owns as +0.0 ;
 *      [workspace u8, 16-byte aligned: md_conv2d_grouped_bwd_weight_workspace_bytes(P, groups, k) bytes; without it the library's
 *      per-stream scratch pool serves]
 * extra: md_conv2d_grouped_attrs, required.
 * The first launch is md_conv_bwd_weight's kernel with the group as a grid dimension (one 16-row MFMA tile per group, rows >= cout[g]
 * zero), the second sums the slabs in that operator's fixed order: the same slabs S, n and L(P) (minddet_hip_convbwd.h), the same bound
 * |dw - exact| <= L(P) 2^-24 sum_p |dy x|.  Group g's rows of dw and db equal, bit for bit, what md_conv_bwd_weight returns for that group
 * alone (kernel k, korder 0, cin 64, x_c_off + 64 g, dy_c_off = y_off[g], cout[g]).
 * 2: as md_conv2d_grouped_bwd_data where it applies (x in the place of dx and act), and: two groups that share a row of w, dw not
 *    [R, k k 64], db not [R], an output that shares its address with another operand, a workspace that is not 16-byte aligned.
 * 4: P or an operand of 2^31 elements or more, a workspace smaller than documented. */
int md_conv2d_grouped_bwd_weight(MD_AOT_ARGS);
extern int64_t md_conv2d_grouped_bwd_weight_workspace_bytes(int64_t P, int64_t groups, int64_t k);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_GROUPEDBWD_H_ */
