/*
 * minddet_hip_train.h -- C ABI of the training-step operators of libminddet_hip.so behind the losses: the weight gradient of a
 * pointwise (1x1) convolution (csrc/convbwd.hip) and the reference's Adam step with its global-norm clip (csrc/optim.hip;
 * minddet/models/centerpoint/det3d_ms/solver/custom_adam.py:590-668 Adam.construct, :188-222 the dense update P.Adam stands for).
 * With them a head whose last layer is a 1x1 conv trains on the device: md_*_loss_grad -> md_conv1x1_bwd_weight -> md_grad_sumsq ->
 * md_adam_step, no host read, no floating-point atomic, no launch that waits on another workgroup.
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 */
#ifndef MINDDET_HIP_TRAIN_H_
#define MINDDET_HIP_TRAIN_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_CONV1X1_BWD_MAX_CIN 1024
#define MD_CONV1X1_BWD_MAX_COUT 256
#define MD_CONV1X1_BWD_SLAB_MIN 256    /* pixels: the smallest slab one workgroup of the first launch reduces */
#define MD_CONV1X1_BWD_MAX_SLABS 256   /* the slab grows with P so that there are never more */
#define MD_CONV1X1_BWD_SUM_WAYS 8      /* the second launch sums the slabs in this many interleaved chains, then the chains in order */

typedef struct md_conv1x1_bwd_attrs {
    int32_t cin;        /* input channels of the layer: a multiple of 8, <= MD_CONV1X1_BWD_MAX_CIN */
    int32_t cout;       /* output channels of the layer: 1 .. MD_CONV1X1_BWD_MAX_COUT */
    int32_t x_c_off;    /* the layer reads channels [x_c_off, x_c_off + cin) of x */
    int32_t dy_c_off;   /* the layer's outputs are channels [dy_c_off, dy_c_off + cout) of dy */
    int32_t reserved0;  /* must be 0 */
} md_conv1x1_bwd_attrs;

/* Weight and bias gradient of a pointwise convolution y[p, o] = sum_i w[o, i] x[p, i] + b[o] over the P = N H W pixels p:
 *   dw[o, i] = sum_p dy[p, o] x[p, i],   db[o] = sum_p dy[p, o]          (o < cout, i < cin)
 * in : x[N,H,W,Cx] bf16, dy[N,H,W,Cy] f32 (what md_*_loss_grad writes)
 * out: dw[rows,kpad] f32 (the shape of a 1x1 layer's packed weight: rows >= cout, kpad >= cin; every element is written, rows >= cout
 *      and columns >= cin as +0.0), db[rowsb] f32 or NULL (rowsb >= cout; elements >= cout +0.0) ;
 *      [workspace u8, 16-byte aligned: md_conv1x1_bwd_weight_workspace_bytes(P, cin, cout) bytes; without it the library's per-stream
 *      scratch pool serves]
 * extra: md_conv1x1_bwd_attrs, required.
 *
 * Arithmetic: the fp32 MFMA (v_mfma_f32_16x16x4_f32) on dy as it is and on x widened to fp32 (exact): dy enters the product with all
 * 24 significant bits, every product is rounded once into an fp32 accumulator.  Neither operand is transposed on the way in: the MFMA's
 * reduction index lies ACROSS lanes, so a lane loads its pixel's channels as they lie in memory (16 bytes of x per load, one load per
 * eight MFMAs) and the MFMA's column index is a permutation of the channels.
 * Order of the additions (fixed: the result is the same from call to call and from stream to stream).  S = max(MD_CONV1X1_BWD_SLAB_MIN,
 * 16 ceil(ceil(P / MD_CONV1X1_BWD_MAX_SLABS) / 16)) pixels are one slab, n = ceil(P / S) slabs.  First launch: each of the four waves of
 * a workgroup takes every fourth group of four pixels of the slab into its accumulators (at most S / 4 products in a chain), the waves
 * are added in order (3 additions), the workgroup stores its partial block to the workspace.  Second launch: per element,
 * MD_CONV1X1_BWD_SUM_WAYS interleaved chains over the slabs (ceil(n / 8) additions each), then the chains in order (7 additions).
 * The longest chain of fp32 roundings behind an element is therefore
 *   L(P) = S / 4 + 3 + ceil(n / 8) + 7
 * and |dw - exact| <= L(P) 2^-24 sum_p |dy x| (db: the same with x = 1).
 * 2: an extent other than documented, N, H or W < 1, cin or cout < 1, a channel range outside x or dy, reserved0 != 0, an output that
 *    shares its address with another operand, a workspace that is not 16-byte aligned.
 * 4: cin % 8 != 0, cin > MD_CONV1X1_BWD_MAX_CIN, cout > MD_CONV1X1_BWD_MAX_COUT, P or an operand of 2^31 elements or more, a workspace
 *    smaller than documented. */
int md_conv1x1_bwd_weight(MD_AOT_ARGS);
extern int64_t md_conv1x1_bwd_weight_workspace_bytes(int64_t P, int64_t cin, int64_t cout);

#define MD_GRAD_SUMSQ_CHUNK 4096       /* elements per block partial */
#define MD_GRAD_SUMSQ_MAX_BLOCKS 1024  /* beyond it a workgroup takes every 1024th chunk */
#define MD_ADAM_MAX_SUMSQ 1024         /* K of md_adam_step */

/* Sum of squares of a flat gradient, in float64, in a fixed order (the result is the same from call to call).
 * in : grad[n] f32, n >= 1
 * out: sumsq[1] f64 ; [workspace u8, 8-byte aligned: md_grad_sumsq_workspace_bytes(n) bytes, or the scratch pool]
 * Two launches: block partials (lane t of workgroup b adds elements 4096 c + t + 256 k of its chunks c = b, b + 1024, ..., then the
 * fixed-order block sum of the losses), then one workgroup over the partials in the same way.
 * 2: an extent other than documented, n < 1, a workspace that is not 8-byte aligned.  4: n >= 2^31, a workspace smaller than documented. */
int md_grad_sumsq(MD_AOT_ARGS);
extern int64_t md_grad_sumsq_workspace_bytes(int64_t n);

typedef struct md_adam_attrs {
    double lr, beta1, beta2;
    double beta1_power, beta2_power;   /* the host's running products prod beta1_t, prod beta2, this step included (kept in fp32 as the
                                          reference's Parameters are); both in [0, 1) */
    double eps, weight_decay;
    double max_norm;                   /* > 0 where sumsq is given; not read without it */
    double grad_scale;                 /* scale_grad's factor (1 / loss scale) */
    double reserved0;                  /* must be 0 */
} md_adam_attrs;

/* Adam.construct (custom_adam.py:590-668) for one flat range, one launch: the global-norm clip, decay_weight, scale_grad and the dense
 * update of :188-222 (P.Adam's formula, :215-218).
 * in : grad[n] f32, sumsq[K] f64 or NULL (the squared norms of every range that is clipped together, e.g. md_grad_sumsq's output;
 *      NULL: no clipping, the plain nn.Adam of pointpillars/train.py:76-93)
 * in / out: param[n] f32, m[n] f32, v[n] f32
 * out: shadow[ns] bf16 or NULL, ns <= n: bf16 (round to nearest even) of the new param[0, ns)
 * extra: md_adam_attrs, required.
 *   total = sqrt(sum_k sumsq[k]) ; coef = max_norm / (total + 1e-6), applied only if coef < 1
 *   g  = grad coef (if clipping) ; g = g + weight_decay param ; g = g grad_scale
 *   m' = beta1 m + (1 - beta1) g ;  v' = beta2 v + (1 - beta2) (g g)
 *   lr_t = lr sqrt(1 - beta2_power) / (1 - beta1_power) ;  param' = param - lr_t (m' / (sqrt(v') + eps))
 * Arithmetic (a choice: MindSpore's Adam kernel is not in the reference): every term in float64 from the fp32 operands, in the order
 * written; m', v' and param' are each rounded once to fp32 (param' from the unrounded m', v').  A zero gradient on zero state leaves
 * param as it is and m, v at +0.0.
 * 2: an extent other than documented, n < 1, ns > n, K < 1, a non-finite attribute, lr < 0, beta1 or beta2 outside [0, 1), a power
 *    outside [0, 1), eps < 0, max_norm <= 0 with sumsq given, grad_scale < 0, reserved0 != 0, an output that shares its address with
 *    grad, sumsq or another output.
 * 4: n >= 2^31, K > MD_ADAM_MAX_SUMSQ. */
int md_adam_step(MD_AOT_ARGS);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_TRAIN_H_ */
