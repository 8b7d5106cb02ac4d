/*
 * minddet_hip_convbwd.h -- C ABI of the two conv-backward operators of libminddet_hip.so that carry a gradient below a head's last
 * layer (csrc/convbwd.hip): the weight gradient of a k x k convolution (k = 1 or 3, stride 1, "same" padding) and the data gradient of a
 * pointwise convolution behind a ReLU.  With md_conv1x1_bwd_weight and md_adam_step (minddet_hip_train.h) a head of a 3x3 conv + ReLU
 * and a 1x1 conv trains on the device: md_cn_loss_grad -> md_conv_bwd_weight (k = 1) -> md_conv1x1_bwd_data -> md_conv_bwd_weight
 * (k = 3) -> md_adam_step, no host read, no floating-point atomic, no launch that waits on another workgroup.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 */
#ifndef MINDDET_HIP_CONVBWD_H_
#define MINDDET_HIP_CONVBWD_H_

#include "minddet_hip_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_CONV_BWD_MAX_CIN_K1 1024   /* = MD_CONV1X1_BWD_MAX_CIN */
#define MD_CONV_BWD_MAX_CIN_K3 256    /* 9 x 256 = 2304 virtual columns */
#define MD_CONV_BWD_MAX_COUT 256      /* = MD_CONV1X1_BWD_MAX_COUT */
#define MD_CONV_BWD_MAX_BLOCKS 4

typedef struct md_conv_bwd_block {
    int32_t row0, rows;   /* output channels [row0, row0 + rows) of the layer, inside [0, cout) */
    int32_t col0, cols;   /* input channels [col0, col0 + cols) of the layer, inside [0, cin) */
} md_conv_bwd_block;

typedef struct md_conv_bwd_attrs {
    int32_t cin;        /* input channels of the layer: a multiple of 8, <= MD_CONV_BWD_MAX_CIN_K1 (kernel 1) / _K3 (kernel 3) */
    int32_t cout;       /* output channels of the layer: 1 .. MD_CONV_BWD_MAX_COUT */
    int32_t x_c_off;    /* the layer reads channels [x_c_off, x_c_off + cin) of x */
    int32_t dy_c_off;   /* the layer's outputs are channels [dy_c_off, dy_c_off + cout) of dy */
    int32_t kernel;     /* 1 or 3: a kernel x kernel conv, stride 1, pad (kernel - 1) / 2 */
    int32_t korder;     /* column order of dw: 0 (tap, channel), 1 (channel / 64, tap, channel % 64); 1 needs cin % 64 == 0 */
    int32_t n_blocks;   /* 0: dense; 1 .. MD_CONV_BWD_MAX_BLOCKS: only the (output, input) channel pairs inside a block are live */
    md_conv_bwd_block blocks[4];   /* MD_CONV_BWD_MAX_BLOCKS of them; the first n_blocks are read */
    int32_t reserved0;  /* must be 0 */
} md_conv_bwd_attrs;

/* Weight and bias gradient of y[p, o] = sum_t sum_i w[o, t, i] x[p + d_t, i] + b[o] over the P = N H W pixels p = (n, h, w), tap
 * t = kernel ky + kx with the offset d_t = (ky - pad, kx - pad) rows and columns, x = 0 where p + d_t leaves p's own image:
 *   dw[o, col(t, i)] = sum_p dy[p, o] x[p + d_t, i],   db[o] = sum_p dy[p, o]          (o < cout, i < cin, t < kernel^2)
 *   col(t, i) = t cin + i                                       (korder 0)
 *   col(t, i) = (i / 64) (kernel^2 64) + t 64 + i % 64          (korder 1)
 * the two K orders of a packed conv weight (md_conv2d_attrs.korder), so dw has the layout of the layer's pack.
 * in : x[N,H,W,Cx] bf16, dy[N,H,W,Cy] f32
 * out: dw[rows,kpad] f32 (rows >= cout, kpad >= kernel^2 cin; every element is written, rows >= cout and columns >= kernel^2 cin as
 *      +0.0), db[rowsb] f32 or NULL (rowsb >= cout; elements >= cout +0.0) ;
 *      [workspace u8, 16-byte aligned: md_conv_bwd_weight_workspace_bytes(P, cin, cout, kernel) bytes; without it the library's
 *      per-stream scratch pool serves]
 * extra: md_conv_bwd_attrs, required.
 * Blocks: with n_blocks > 0 an element of dw whose (o, i) lies in none of the blocks is written as +0.0 (every tap of it); db is not
 * affected.  A block-diagonal fused layer stays block-diagonal under training.  The mask acts where the second launch stores, the
 * products of the first launch are those of the dense layer.
 *
 * Arithmetic and order of the additions: those of md_conv1x1_bwd_weight (minddet_hip_train.h), the same kernel body with (t, i) as one
 * column axis of kernel^2 cin columns: the fp32 MFMA on dy as it is and on x widened exactly, a lane group of eight columns belongs to
 * one tap and loads its own shifted pixel under its own in-image predicate.  S = max(MD_CONV1X1_BWD_SLAB_MIN,
 * 16 ceil(ceil(P / MD_CONV1X1_BWD_MAX_SLABS) / 16)) pixels of dy are one slab, n = ceil(P / S) slabs; per slab four waves with S / 4
 * products in a chain each, added in order (3 additions); the second launch sums the slabs in MD_CONV1X1_BWD_SUM_WAYS interleaved
 * chains (ceil(n / 8) additions each), then the chains in order (7 additions):
 *   L(P) = S / 4 + 3 + ceil(n / 8) + 7
 * and |dw - exact| <= L(P) 2^-24 sum_p |dy x| (db: the same with x = 1).  The result is the same from call to call and from stream to
 * stream.  With kernel 1, korder 0 and n_blocks 0 the results are those of md_conv1x1_bwd_weight bit for bit.
 * 2: an extent other than documented, N, H or W < 1, cin or cout < 1, a channel range outside x or dy, reserved0 != 0, an output that
 *    shares its address with another operand, a workspace that is not 16-byte aligned, kernel not 1 or 3, korder not 0 or 1, n_blocks
 *    outside [0, MD_CONV_BWD_MAX_BLOCKS], a block with rows or cols < 1 or outside [0, cout) x [0, cin).
 * 4: cin % 8 != 0, cin above the limit of its kernel, cout > MD_CONV_BWD_MAX_COUT, korder 1 with cin % 64 != 0, P or an operand of 2^31
 *    elements or more, a workspace smaller than documented. */
int md_conv_bwd_weight(MD_AOT_ARGS);
extern int64_t md_conv_bwd_weight_workspace_bytes(int64_t P, int64_t cin, int64_t cout, int64_t kernel);

#define MD_CONV1X1_BWD_DATA_MAX_CIN 1024
#define MD_CONV1X1_BWD_DATA_MAX_COUT 256

typedef struct md_conv1x1_bwd_data_attrs {
    int32_t cin;        /* input channels of the layer: a multiple of 8, <= MD_CONV1X1_BWD_DATA_MAX_CIN */
    int32_t cout;       /* output channels of the layer: 1 .. MD_CONV1X1_BWD_DATA_MAX_COUT */
    int32_t dy_c_off;   /* the layer's outputs are channels [dy_c_off, dy_c_off + cout) of dy */
    int32_t dx_c_off;   /* the gradient is written to channels [dx_c_off, dx_c_off + cin) of dx */
    int32_t act_c_off;  /* the layer's input is channels [act_c_off, act_c_off + cin) of act; 0 without act */
    int32_t reserved0;  /* must be 0 */
} md_conv1x1_bwd_data_attrs;

/* Input gradient of a pointwise convolution y[p, o] = sum_i w[o, i] x[p, i] + b[o], optionally through the ReLU that made x:
 *   dx[p, i] = sum_{o < cout} dy[p, o] w[o, i]                    (i < cin)
 *   with act: dx[p, i] = +0.0 unless act[p, act_c_off + i] > 0    (a -0, a negative value or a NaN in act gives +0.0)
 * in : dy[N,H,W,Cy] f32, w[rows,kpad] bf16 (the layer's pack, korder 0: rows >= cout, kpad >= cin; the weights the forward pass read),
 *      act[N,H,W,Ca] bf16 or NULL (the ReLU's output, the tensor the forward pass gave the layer)
 * out: dx[N,H,W,Cdx] f32: channels [dx_c_off, dx_c_off + cin) are written, every other channel is left as it was
 * extra: md_conv1x1_bwd_data_attrs, required.
 * One launch, no workspace: a workgroup keeps the [cout][128] tile of w of its 128 input channels in LDS and streams the pixels past it,
 * 16 per wave and step.  The fp32 MFMA (v_mfma_f32_16x16x4_f32) on dy as it is and on w widened to fp32 (exact); the reduction index o
 * is the fast axis of dy, so dy is not transposed.  Order of the additions (fixed): one accumulator per element, o ascending, four per
 * MFMA; the MFMA is an fp32 fma chain in o, every product rounded once into the accumulator.  The chain of roundings behind an element
 * is
 *   Ld(cout) = cout
 * and |dx - exact| <= Ld 2^-24 sum_o |dy w|.  The result is the same from call to call and from stream to stream.
 * 2: an extent other than documented, N, H or W < 1, cin or cout < 1, a channel range outside dy, dx or act, rows < cout or kpad < cin,
 *    act_c_off != 0 without act, reserved0 != 0, dx at the address of another operand.
 * 4: cin % 8 != 0, cin > MD_CONV1X1_BWD_DATA_MAX_CIN, cout > MD_CONV1X1_BWD_DATA_MAX_COUT, P or an operand of 2^31 elements or more. */
int md_conv1x1_bwd_data(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_CONVBWD_H_ */
