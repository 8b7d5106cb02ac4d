/*
 * minddet_hip_chain.h -- C ABI of the pointwise-chain op of libminddet_hip.so: the tail of one ResNet bottleneck block and the head of
 * the next one in a single launch (stage 2 of ResNet-50 / 101: 128 mid channels, 512 block channels).
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions"), which this header includes.
 */
#ifndef MINDDET_HIP_CHAIN_H_
#define MINDDET_HIP_CHAIN_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* conv3 (1x1, 128 -> 512) + residual + ReLU of an identity bottleneck block, and conv1 (1x1, 512 -> 128) + ReLU of the block behind it,
 * computed from the 512-channel tile while it is on chip: y is written once and not read back.
 * in : t2[N,H,W,128] bf16, res[N,H,W,512] bf16, w3[512,128] bf16, b3[512] f32, w1[128,512] bf16, b1[128] f32 (BN folded, K-major rows, as
 *      md_conv2d takes them)
 * out: y[N,H,W,512] bf16, t1[N,H,W,128] bf16.   extra: not read.
 *   y  = bf16(relu(bf16(w3 . t2 + b3) + res))      -- the roundings of md_conv2d with a residual and relu = 1
 *   t1 = bf16(relu(w1 . y + b1))                   -- md_conv2d with relu = 1 on the stored (bf16) y
 * Both results are bit-identical to those two md_conv2d calls, and both are held to a float64 reference of these rounding points
 * (tests/conv_contract.py reference_pw_chain) by tests/test_pw_chain_gpu.py: test_exact_regime_both_outputs_bit_for_bit and
 * test_gaussian_regime_y_and_t1_within_the_float64_contract.  All activations are whole contiguous NHWC tensors: an operand with
 * another channel count (a channel slice of a wider tensor) is refused.
 * 2: channel counts other than 128 / 512 / 128, weight or bias shapes other than the above, N H W not the same in every activation,
 *    y or t1 overlapping t2, res or each other (the residual of a tile is fetched while earlier tiles are stored: in place is not safe).
 * 4: N H W >= 2^31.  (No byte limit: every access is addressed from a 64-bit base per 32-pixel tile.) */
int md_pw_chain(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_CHAIN_H_ */
