// image_sample.h -- the bilinear sampler of the image operators, stated once: md_image_preprocess (preproc.hip) and md_cn_aug_image
// (cnaug.hip) read a source pixel through these functions, so the two give the same bits on the same matrix.  Device code only.
// Every multiply-add is spelled (fmaf, contraction off), so the bits do not depend on the translation unit's contraction mode: the
// fused operations are the ones md_image_preprocess has always run (tests/cnaug_contract.py restates the sequence in numpy).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device.h"

namespace md {

// v[0..2] += the bilinear sample of the 3-channel uint8 image `base` (row pitch `pitch` pixels, valid extent h x w) at the source
// position of output pixel (x, y) under m[6]: sx = fma(m0, x, m1 y) + m2, sy = fma(m4, y, m3 x) + m5.  In grey levels (0..255), fp32:
// v = fma(wy wx, p, v) over the taps in the order (y0, x0), (y0, x1), (y1, x0), (y1, x1); a tap outside h x w adds nothing
// (BORDER_CONSTANT, value 0).  A source position outside (-1, w) x (-1, h) touches no pixel: huge, infinite and NaN positions stop
// here, before the conversion to int (undefined for them), and read as the border value.
__device__ __forceinline__ void sample_bilinear(const uint8_t *__restrict__ base, int pitch, int h, int w, const float *__restrict__ m, int x, int y,
                                                float (&v)[3]) {
#pragma clang fp contract(off)
    const float sx = __builtin_fmaf(m[0], (float)x, m[1] * (float)y) + m[2];
    const float sy = __builtin_fmaf(m[4], (float)y, m[3] * (float)x) + m[5];
    if (sx > -1.f && sx < (float)w && sy > -1.f && sy < (float)h) {
        const float xf = floorf(sx), yf = floorf(sy);
        const int x0 = (int)xf, y0 = (int)yf;
        const float lx = sx - xf, ly = sy - yf;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int yy = y0 + (q >> 1), xx = x0 + (q & 1);
            const float wt = ((q >> 1) ? ly : 1.f - ly) * ((q & 1) ? lx : 1.f - lx);
            if ((unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w) {
                const uint8_t *p = base + ((size_t)yy * pitch + xx) * 3;
                v[0] = __builtin_fmaf(wt, (float)p[0], v[0]);
                v[1] = __builtin_fmaf(wt, (float)p[1], v[1]);
                v[2] = __builtin_fmaf(wt, (float)p[2], v[2]);
            }
        }
    }
}

// the network's input value of a sample v in grey levels, norm = mean[3] then std[3] in units of the 0..1 image: fma(v, 1 / 255, -mean) / std
__device__ __forceinline__ float normalised_level(float v, const float *__restrict__ norm, int c) {
#pragma clang fp contract(off)
    return __builtin_fmaf(v, 1.0f / 255.0f, -norm[c]) / norm[3 + c];
}

// one pixel of the padded output: 3 values and a zero as 4 bf16, and 4 more zeros where C = 8
__device__ __forceinline__ void store_pixel(uint16_t *dst, const float (&v)[3], int C) {
    *reinterpret_cast<uint2 *>(dst) = make_uint2(pk_bf16(v[0], v[1]), pk_bf16(v[2], 0.f));
    if (C == 8) *reinterpret_cast<uint2 *>(dst + 4) = make_uint2(0u, 0u);
}

}  // namespace md
