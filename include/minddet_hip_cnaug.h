/*
 * minddet_hip_cnaug.h -- C ABI of the CenterNet training input of libminddet_hip.so: the training branch of COCOHP.preprocess_fn
 * (centernet/src/dataset.py:278-315) with color_aug (centernet/src/image.py:208-253), from the values the reference drew to the
 * normalised network input, which the reference runs per image on the host with cv2 and numpy.  The target step behind it is
 * md_cn_assign_targets (minddet_hip_cn.h); the inference warp is md_image_preprocess (minddet_hip.h), whose sampler and output
 * layout md_cn_aug_image shares (csrc/image_sample.h).
 * Same calling convention, error codes and argument-check rule as include/minddet_hip.h ("Conventions").
 *
 * As in minddet_hip_pcaug.h: the ops contain no random number generator (every draw is a float64 operand), no floating-point atomics,
 * no memset, no host read; two calls give the same bits, on any stream.  No output may share its address with an input or with another
 * output: such a call is refused with rc 2.  tests/cnaug_contract.py states the ops in numpy.
 *
 * Reference quirks
 *  (a) saturation_ scales `gs` in place through a view (image.py:229: blend_ runs image2 *= 1 - alpha on gs[:, :, None]).  Harmless:
 *      gs is read by nobody afterwards (gs_mean was taken before, contrast_ reads gs_mean only).  The op reads the unscaled grey.
 *  (b) the alphas are Python floats and the image is fp32, so numpy runs every step of brightness_ / contrast_ / saturation_ as an
 *      fp32 loop; lighting_ adds a float64 vector to the fp32 image (one more fp32 rounding per element).  The op runs the chain in
 *      float64 and rounds once; the contract derives the forward bound of the reference's fp32 sequence against that chain.
 *  (c) cv2.warpAffine returns uint8, i.e. grey levels rounded to integers, and interpolates in 1/32-pixel fixed point.  This sampler
 *      interpolates in fp32 and does not round to grey levels (as md_image_preprocess).  Unpinned, cv2 is absent here.
 *  (d) cv2.cvtColor(BGR2GRAY) is cv2's own code: the grey weights 0.114 B + 0.587 G + 0.299 R are the documented ones, its arithmetic
 *      is unpinned.
 *  (e) cv2.getAffineTransform is cv2's own solve: unpinned.  The op evaluates the closed form below.
 * Not built (the Python layer refuses them with ValueError; the ABI has no operand for them): rot != 0, keep_res, a down_ratio
 * that differs between the two axes.
 */
#ifndef MINDDET_HIP_CNAUG_H_
#define MINDDET_HIP_CNAUG_H_

#include "minddet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MD_CNAUG_MAX_BATCH 65535 /* B: one workgroup row per sample */
#define MD_CNAUG_GREY_CHUNK 2048 /* output pixels per partial sum of the grey pass (the workspace formula) */

typedef struct md_cn_aug_transform_attrs {
    int32_t rand_crop;   /* != 0: the rand_crop branch (dataset.py:289-294), else the scale / shift branch (:295-300) */
    double scale, shift; /* data_opt.scale (sf) and data_opt.shift (cf); finite */
    double flip_prop;    /* in [0, 1]: the sample is flipped where its fourth draw is below it */
    int32_t in_h, in_w;  /* input_res_train; >= 1 */
    int32_t down_ratio;  /* >= 1: the output map is (in_w / down_ratio) x (in_h / down_ratio), integer division */
} md_cn_aug_transform_attrs;
/* The random block of preprocess_fn (dataset.py:278-306) and its two get_affine_transform calls (:307, :320), one lane per sample.
 * in : sizes[B,2] i32 = (h, w) of each source image; draws[B,4] f64 = the values the reference drew:
 *      rand_crop: (the chosen element of np.arange(0.6, 1.4, 0.1), randint for c[0], randint for c[1], random() of the flip);
 *      else     : (randn() of c[0], randn() of c[1], randn() of s -- the order of :298-300 --, random() of the flip)
 * out: mat_in[B,6] f32 = the matrix md_image_preprocess documents (output pixel -> source pixel) for the STORED, unflipped image: the
 *      flip img[:, ::-1] is folded in as sx -> w - 1 - sx; trans_out[B,6] f64 = trans_output (source -> output map), as
 *      CenterNetTargets consumes it; flip_width[B] i32 = w where the sample is flipped, else 0
 * extra: md_cn_aug_transform_attrs, required.
 * Value types, step by step as the reference holds them (contraction off; fl32 = one rounding to fp32):
 *   cx = fl32(w / 2), cy = fl32(h / 2), s = max(h, w)                                       (c an fp32 pair, s a float64)
 *   rand_crop: s = s d0; cx = fl32(d1); cy = fl32(d2)
 *   else     : cx = fl32(cx + s clip(d0 cf, -2 cf, 2 cf)); cy = fl32(cy + s clip(d1 cf, -2 cf, 2 cf)) with the old s;
 *              s = s clip(d2 sf + 1, 1 - sf, 1 + sf);   clip(v, lo, hi) = min(max(v, lo), hi)
 *   flipped = d3 < flip_prop; flipped: cx = fl32(fl32(fl32(w) - cx) - 1)                    (fp32, :305)
 *   s32 = fl32(s)                                                                            (image.py:29-30)
 * With rot = 0 the three-point solve of get_affine_transform has a closed form, evaluated in float64 on cx, cy, s32:
 *   trans_out: k = out_w / s32;  [k, 0, out_w / 2 - k cx;  0, k, out_h / 2 - k cy]
 *   mat_in   : r = s32 / in_w;  ox = cx - r (in_w / 2);  oy = cy - r (in_h / 2);
 *              not flipped [r, 0, ox; 0, r, oy], flipped [-r, 0, (w - 1) - ox; 0, r, oy], each entry rounded once to fp32
 * (the reference's own points are fp32 and cv2 solves them in float64: the closed form differs from that solve by the roundings of
 * the three points, bounded in tests/cnaug_contract.py).
 * A size < 1 is an argument error that only the device can see: the three outputs of that sample are zeros, nothing is read back.
 * 2: B differs between operands, an extent other than documented, a non-finite attribute, flip_prop outside [0, 1], in_h, in_w or
 * down_ratio < 1, in_w or in_h below down_ratio.  4: B > MD_CNAUG_MAX_BATCH. */
int md_cn_aug_transform(MD_AOT_ARGS);

typedef struct md_cn_aug_image_attrs {
    int32_t out_h, out_w, pad_lo, pad_hi;
} md_cn_aug_image_attrs;
/* cv2.warpAffine + / 255 + color_aug + (inp - mean) / std + the layout (dataset.py:308-315), per-sample source extent.
 * in : img[B,Hs,Ws,3] u8 (BGR; the samples padded to a common extent); sizes[B,2] i32 = (h, w) of each sample, clamped to
 *      [0, Hs] x [0, Ws]: a source position outside the sample's own h x w is border, whatever lies in the padding;
 *      mat_in[B,6] f32 (md_cn_aug_transform's); norm[6] f32 = mean[3], std[3] of the 0..1 image;
 *      colour[B,8] f64 or NULL = (alpha of brightness_, of contrast_, of saturation_; the three lighting terms
 *      dot(eig_vec, eig_val * alpha)[c] per channel, multiplied out; the order of the three functions; one spare slot).  The order is
 *      the index 0..5 of the permutation in lexicographic order with 0 = brightness_, 1 = contrast_, 2 = saturation_:
 *      0 = (b, c, s), 1 = (b, s, c), 2 = (c, b, s), 3 = (c, s, b), 4 = (s, b, c), 5 = (s, c, b).  NULL: no colour augmentation
 * out: y[B, pad_lo + out_h + pad_hi, pad_lo + out_w + pad_hi, C = 4 | 8] bf16, md_image_preprocess's output layout; the border and the
 *      spare channels are exactly +0 ; [workspace u8, 8-byte aligned: md_cn_aug_image_workspace_bytes(B, out_h, out_w) bytes; never more
 *      than 8 B ((out_h out_w + 2047) / 2048 + 1); without it the library's per-stream scratch pool serves; not touched when colour
 *      is NULL]
 * extra: md_cn_aug_image_attrs, required.
 * Per output pixel of the image area:
 *   1. v[c] = the fp32 bilinear sample in grey levels, exactly md_image_preprocess's (csrc/image_sample.h)
 *   colour NULL: y = fma(v, 1 / 255, -mean) / std in fp32, md_image_preprocess's expression: the two ops give the same bits.
 *   2. x[c] = fl32(v[c] (1 / 255f)); grey g = (0.114 x0 + 0.587 x1) + 0.299 x2 in float64; gs_mean = the mean of g over the sample's
 *      out_h out_w pixels, summed in float64 in a fixed order (a partial sum per 2048 pixels, then a fixed-order finish)
 *   3. in float64, in the given order: brightness x = x a;  contrast x = a x + (1 - a) gs_mean;  saturation x = a x + (1 - a) g (g: the
 *      grey of the pixel before any of the three, quirk (a));  then lighting x = x + l[c]
 *   4. one rounding to fp32, then y = (x - mean) / std in fp32, then bf16 (round to nearest even)
 * An order that is not one of 0..5 is an argument error that only the device can see: the three functions are skipped for that
 * sample (the lighting terms still apply); nothing is read back.  Non-finite matrix entries give the black level, as in
 * md_image_preprocess.
 * Launches: the grey pass, its finish, the output pass (which samples the uint8 source again: no fp32 intermediate image).
 * 2: an extent other than documented, C not 4 or 8, a workspace that is not 8-byte aligned, an output that shares its address with an
 * input.  4: an operand of 2^30 elements or more, B > MD_CNAUG_MAX_BATCH, a workspace smaller than documented. */
int md_cn_aug_image(MD_AOT_ARGS);
int64_t md_cn_aug_image_workspace_bytes(int64_t B, int64_t out_h, int64_t out_w);

#ifdef __cplusplus
}
#endif
#endif /* MINDDET_HIP_CNAUG_H_ */
