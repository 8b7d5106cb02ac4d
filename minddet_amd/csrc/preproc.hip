// preproc.hip -- image pre-processing on the device: affine warp (bilinear, constant-0 border) + normalisation +
// layout, uint8 HWC -> bf16 in the network's input layout.  SURVEY 8(f) rank 2: "the step immediately before the path".
//
// What it replaces: the host path of minddet/models/centernet/src/dataset.py:223-256 (cv2.resize + cv2.warpAffine with
// flags=INTER_LINEAR, then (img / 255 - mean) / std) together with the on-device ImagePreProcess cell
// (centernet/src/centernet_det.py:240-262: cast, (image - mean) / std, transpose).  The caller passes the 2x3 matrix that
// maps OUTPUT pixel coordinates to SOURCE pixel coordinates (the inverse of get_affine_transform's matrix,
// centernet/src/image.py:25-57, composed with the resize).  cv2 interpolates in 1/32-pixel fixed point with 15-bit weight
// tables; this kernel interpolates in fp32 -- cv2 is not installable here, so that difference (<= 1/64 pixel of sampling
// position, <= 1 grey level) is documented and parity is unpinned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aot.h"
#include "device.h"
#include "image_sample.h"

namespace md {

struct PreArgs {
    const uint8_t *img;   // [N,Hs,Ws,3]
    const float *mat;     // [N,6]: sx = m0 x + m1 y + m2, sy = m3 x + m4 y + m5 (x, y = output pixel)
    const float *norm;    // mean[3] then std[3], in units of the 0..1 image
    uint16_t *out;        // [N,Hp,Wp,C] bf16, C = 4 or 8, image area at (pad_lo, pad_lo), everything else zero
    int N, Hs, Ws, Ho, Wo, Hp, Wp, C, pad_lo;
};

// one lane = one output pixel of the PADDED tensor (8 or 16 bytes), so the zero border is written by the same pass
__global__ __launch_bounds__(256) void image_preprocess_kernel(PreArgs a, size_t total) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int xp = (int)(e % a.Wp);
        const int yp = (int)((e / a.Wp) % a.Hp);
        const int n = (int)(e / ((size_t)a.Wp * a.Hp));
        const int x = xp - a.pad_lo, y = yp - a.pad_lo;
        float v[3] = {0.f, 0.f, 0.f};
        const bool inside = (unsigned)x < (unsigned)a.Wo && (unsigned)y < (unsigned)a.Ho;
        if (inside) {
            sample_bilinear(a.img + (size_t)n * a.Hs * a.Ws * 3, a.Ws, a.Hs, a.Ws, a.mat + (size_t)n * 6, x, y, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = normalised_level(v[c], a.norm, c);
        }
        store_pixel(a.out + e * a.C, v, a.C);
    }
}

}  // namespace md

using namespace md;

extern "C" int md_image_preprocess(MD_AOT_ARGS) {
    // in: img[N,Hs,Ws,3] uint8, mat[N,6] f32 (output pixel -> source pixel), norm[6] f32 (mean, std) ;
    // out: y[N, pad_lo + out_h + pad_hi, pad_lo + out_w + pad_hi, C = 4 | 8] bf16 -- extra: md_preprocess_attrs {out_h, out_w, pad_lo, pad_hi}
    Args g(MD_ARGS, 4, 4);
    const md_preprocess_attrs *at = g.attrs<md_preprocess_attrs>(extra);
    g.tensor(0, U8, 4); g.tensor(1, F32, 2); g.tensor(2, F32); g.tensor(3, BF16, 4);
    if (int rc = g.rc()) return rc;
    PreArgs a;
    a.N = (int)g.d(0, 0); a.Hs = (int)g.d(0, 1); a.Ws = (int)g.d(0, 2);
    a.Ho = at->out_h; a.Wo = at->out_w; a.pad_lo = at->pad_lo;
    a.Hp = (int)g.d(3, 1); a.Wp = (int)g.d(3, 2); a.C = (int)g.d(3, 3);
    if (g.d(0, 3) != 3 || g.d(1, 0) != a.N || g.d(1, 1) != 6 || g.numel(2) != 6 || g.d(3, 0) != a.N) return MD_ERR_ARG;
    if ((a.C != 4 && a.C != 8) || a.Ho < 1 || a.Wo < 1 || a.pad_lo < 0 || at->pad_hi < 0 || a.Hp != a.Ho + a.pad_lo + at->pad_hi ||
        a.Wp != a.Wo + a.pad_lo + at->pad_hi)
        return MD_ERR_ARG;
    const size_t total = (size_t)a.N * a.Hp * a.Wp;
    if (total == 0) return MD_OK;
    if (!g.have({0, 1, 2, 3})) return MD_ERR_ARG;
    a.img = (const uint8_t *)params[0]; a.mat = (const float *)params[1]; a.norm = (const float *)params[2];
    a.out = (uint16_t *)params[3];
    const size_t nb = (total + 255) / 256;
    hipLaunchKernelGGL(image_preprocess_kernel, dim3((unsigned)(nb < 0x7fffffffull ? nb : 0x7fffffffull)), dim3(256), 0, (hipStream_t)stream, a, total);
    return launched();
}
