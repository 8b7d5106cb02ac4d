// cnaug.hip -- CenterNet training input on the device (include/minddet_hip_cnaug.h; feeds the stem and md_cn_assign_targets).
//
// What it replaces: the training branch of COCOHP.preprocess_fn (centernet/src/dataset.py:278-315) with color_aug
// (centernet/src/image.py:208-253): the random block, two get_affine_transform calls, cv2.warpAffine, / 255, the colour chain and
// (inp - mean) / std, per image on the host with cv2 and numpy.
//   cn_transform_kernel   one lane per sample: c, s, the flip, mat_in, trans_out, flip_width
//   cn_grey_kernel        (2048 output pixels, sample) per workgroup: the sampler, the pixel's grey in float64, one fixed-order block sum
//                         (loss_common.h block_sums) = one partial in the workspace
//   cn_grey_finish_kernel one workgroup per sample: its partials in a fixed order, gs_mean in the workspace
//   cn_image_kernel       one lane per pixel of the padded output, as image_preprocess_kernel: samples the uint8 source again (it is a
//                         third of an fp32 intermediate image and sits in L2), the colour chain, the normalisation, one 8 / 16-byte store
// LDS: 32 bytes (the block sum) in the two grey kernels, none elsewhere.  No floating-point atomics, no memset.
// The transform and the colour chain in float64 with contraction off; the sampler is image_sample.h's, shared with preproc.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "aot.h"
#include "../../include/minddet_hip_cnaug.h"

#pragma clang fp contract(off)

#include "device.h"
#include "image_sample.h"
#include "loss_common.h"

namespace md {

static_assert(sizeof(md_cn_aug_transform_attrs) == 48 && sizeof(md_cn_aug_image_attrs) == 16, "minddet_hip_cnaug.h: attribute struct layout");

constexpr const char *CNA_F64 = "float64";
constexpr int CNA_MAX_BATCH = MD_CNAUG_MAX_BATCH, CNA_CHUNK = MD_CNAUG_GREY_CHUNK;

// ------------------------------------------------------------------------------------------------ md_cn_aug_transform
struct TransformArgs {
    const int *sizes; const double *draws;
    float *mat_in; double *trans_out; int *flip_width;
    int B, rand_crop, in_h, in_w, out_h, out_w;
    double scale, shift, flip_prop;
};

__device__ __forceinline__ double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

__global__ __launch_bounds__(64) void cn_transform_kernel(TransformArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const int h = a.sizes[2 * b], w = a.sizes[2 * b + 1];
    float *mi = a.mat_in + (size_t)b * 6;
    double *to = a.trans_out + (size_t)b * 6;
    if (h < 1 || w < 1) {
        for (int e = 0; e < 6; ++e) { mi[e] = 0.f; to[e] = 0.0; }
        a.flip_width[b] = 0;
        return;
    }
    const double *d = a.draws + (size_t)b * 4;
    float cx = (float)((double)w / 2.0), cy = (float)((double)h / 2.0);
    double s = (double)max(h, w);
    if (a.rand_crop) {
        s = s * d[0];
        cx = (float)d[1];
        cy = (float)d[2];
    } else {
        const double cf = a.shift, sf = a.scale;
        cx = (float)((double)cx + s * clipd(d[0] * cf, -2.0 * cf, 2.0 * cf));
        cy = (float)((double)cy + s * clipd(d[1] * cf, -2.0 * cf, 2.0 * cf));
        s = s * clipd(d[2] * sf + 1.0, 1.0 - sf, 1.0 + sf);
    }
    const bool flipped = d[3] < a.flip_prop;
    if (flipped) cx = ((float)w - cx) - 1.0f;
    const double s32 = (double)(float)s, dcx = (double)cx, dcy = (double)cy;
    const double k = (double)a.out_w / s32;
    to[0] = k; to[1] = 0.0; to[2] = (double)a.out_w * 0.5 - k * dcx;
    to[3] = 0.0; to[4] = k; to[5] = (double)a.out_h * 0.5 - k * dcy;
    const double r = s32 / (double)a.in_w;
    const double ox = dcx - r * ((double)a.in_w * 0.5), oy = dcy - r * ((double)a.in_h * 0.5);
    mi[0] = (float)(flipped ? -r : r); mi[1] = 0.f; mi[2] = (float)(flipped ? (double)(w - 1) - ox : ox);
    mi[3] = 0.f; mi[4] = (float)r; mi[5] = (float)oy;
    a.flip_width[b] = flipped ? w : 0;
}

// ------------------------------------------------------------------------------------------------ md_cn_aug_image
struct ImageArgs {
    const uint8_t *img; const int *sizes; const float *mat; const float *norm; const double *colour;
    uint16_t *out; double *part, *mean;
    int Hs, Ws, Ho, Wo, Hp, Wp, C, pad_lo, nblk;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the sample's pixel (x, y) of the image area in grey levels
__device__ __forceinline__ void sample_of(const ImageArgs &a, int b, int x, int y, float (&v)[3]) {
    const int h = clampi(a.sizes[2 * b], 0, a.Hs), w = clampi(a.sizes[2 * b + 1], 0, a.Ws);
    sample_bilinear(a.img + (size_t)b * a.Hs * a.Ws * 3, a.Ws, h, w, a.mat + (size_t)b * 6, x, y, v);
}
// the 0..1 image's fp32 values and their grey (the image is BGR)
__device__ __forceinline__ double grey_of(const float (&v)[3], double (&x)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = (double)(v[c] * (1.0f / 255.0f));
    return (0.114 * x[0] + 0.587 * x[1]) + 0.299 * x[2];
}

__global__ __launch_bounds__(256) void cn_grey_kernel(ImageArgs a) {
    __shared__ double red[4];
    const int b = blockIdx.y, npix = a.Ho * a.Wo, p0 = blockIdx.x * CNA_CHUNK;
    double acc[1] = {0.0};
    for (int k = threadIdx.x; k < CNA_CHUNK; k += 256) {
        const int p = p0 + k;
        if (p < npix) {
            const int y = p / a.Wo, x = p - y * a.Wo;
            float v[3] = {0.f, 0.f, 0.f};
            double xs[3];
            sample_of(a, b, x, y, v);
            acc[0] += grey_of(v, xs);
        }
    }
    block_sums<1>(acc, red);
    if (threadIdx.x == 0) a.part[(size_t)b * a.nblk + blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(256) void cn_grey_finish_kernel(ImageArgs a) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const double *part = a.part + (size_t)b * a.nblk;
    double acc[1] = {0.0};
    for (int k = threadIdx.x; k < a.nblk; k += 256) acc[0] += part[k];
    block_sums<1>(acc, red);
    if (threadIdx.x == 0) a.mean[b] = acc[0] / (double)(a.Ho * a.Wo);
}

// one lane = one output pixel of the PADDED tensor (8 or 16 bytes), so the zero border is written by the same pass
template <bool COLOUR> __global__ __launch_bounds__(256) void cn_image_kernel(ImageArgs a) {
    const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.Hp * a.Wp) return;
    const int yp = e / a.Wp, xp = e - yp * a.Wp;
    const int x = xp - a.pad_lo, y = yp - a.pad_lo;
    float v[3] = {0.f, 0.f, 0.f};
    if ((unsigned)x < (unsigned)a.Wo && (unsigned)y < (unsigned)a.Ho) {
        sample_of(a, b, x, y, v);
        if (COLOUR) {
            const double *col = a.colour + (size_t)b * 8;
            double xs[3];
            const double g = grey_of(v, xs), mean = a.mean[b];
            // the order index -> the three functions (0 brightness, 1 contrast, 2 saturation); -1: none of them
            const double od = col[6];
            const int perm = (od >= 0.0 && od <= 5.0) ? (int)od : -1;
            const int f0 = perm >> 1, lo = f0 == 0 ? 1 : 0, hi = f0 == 2 ? 1 : 2;
            const int order[3] = {f0, (perm & 1) ? hi : lo, (perm & 1) ? lo : hi};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double xv = xs[c];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int f = perm < 0 ? -1 : order[i];
                    if (f == 0) xv = xv * col[0];
                    else if (f == 1) xv = col[1] * xv + (1.0 - col[1]) * mean;
                    else if (f == 2) xv = col[2] * xv + (1.0 - col[2]) * g;
                }
                xv = xv + col[3 + c];
                v[c] = ((float)xv - a.norm[c]) / a.norm[3 + c];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = normalised_level(v[c], a.norm, c);
        }
    }
    store_pixel(a.out + ((size_t)b * a.Hp * a.Wp + e) * a.C, v, a.C);
}

}  // namespace md

using namespace md;

extern "C" int md_cn_aug_transform(MD_AOT_ARGS) {
    // in : sizes[B,2] i32, draws[B,4] f64 ; out: mat_in[B,6] f32, trans_out[B,6] f64, flip_width[B] i32
    Args a(MD_ARGS, 5, 5);
    const md_cn_aug_transform_attrs *at = a.attrs<md_cn_aug_transform_attrs>(extra);
    a.tensor(0, I32, 2); a.tensor(1, CNA_F64, 2); a.tensor(2, F32, 2); a.tensor(3, CNA_F64, 2); a.tensor(4, I32, 1);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0);
    a.require(B >= 0 && a.d(0, 1) == 2 && a.d(1, 0) == B && a.d(1, 1) == 4 && a.d(2, 0) == B && a.d(2, 1) == 6);
    a.require(a.d(3, 0) == B && a.d(3, 1) == 6 && a.d(4, 0) == B);
    a.require(isfinite(at->scale) && isfinite(at->shift) && at->flip_prop >= 0.0 && at->flip_prop <= 1.0);      // (a NaN fails both)
    a.require(at->in_h >= 1 && at->in_w >= 1 && at->down_ratio >= 1 && at->in_h >= at->down_ratio && at->in_w >= at->down_ratio);
    if (int rc = a.rc()) return rc;
    if (B > CNA_MAX_BATCH) return MD_ERR_SIZE;
    if (B == 0) return MD_OK;
    if (!a.have({0, 1, 2, 3, 4})) return MD_ERR_ARG;
    for (int o = 2; o < 5; ++o)
        for (int k = 0; k < o; ++k)
            if (params[k] == params[o]) return MD_ERR_ARG;
    TransformArgs k;
    k.sizes = (const int *)params[0]; k.draws = (const double *)params[1];
    k.mat_in = (float *)params[2]; k.trans_out = (double *)params[3]; k.flip_width = (int *)params[4];
    k.B = (int)B; k.rand_crop = at->rand_crop != 0; k.in_h = at->in_h; k.in_w = at->in_w;
    k.out_h = at->in_h / at->down_ratio; k.out_w = at->in_w / at->down_ratio;
    k.scale = at->scale; k.shift = at->shift; k.flip_prop = at->flip_prop;
    hipLaunchKernelGGL(cn_transform_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, k);
    return launched();
}

// partial sums per sample of the grey pass of md_cn_aug_image: one per CNA_CHUNK output pixels
static Sz cn_grey_chunks(Sz out_h, Sz out_w) { return (out_h * out_w + (CNA_CHUNK - 1)) / CNA_CHUNK; }
// scratch of md_cn_aug_image: part[B][chunks] f64 at 0, then mean[B] f64
extern "C" int64_t md_cn_aug_image_workspace_bytes(int64_t B, int64_t out_h, int64_t out_w) {
    return any_negative({B, out_h, out_w}) ? -1 : ws_answer((int64_t)(Sz(B) * (cn_grey_chunks(out_h, out_w) + 1) * 8));
}

extern "C" int md_cn_aug_image(MD_AOT_ARGS) {
    // in : img[B,Hs,Ws,3] u8, sizes[B,2] i32, mat_in[B,6] f32, norm[6] f32, colour[B,8] f64 | NULL
    // out: y[B, pad_lo + out_h + pad_hi, pad_lo + out_w + pad_hi, C = 4 | 8] bf16 ; [workspace]
    Args g(MD_ARGS, 6, 7);
    const md_cn_aug_image_attrs *at = g.attrs<md_cn_aug_image_attrs>(extra);
    g.tensor(0, U8, 4); g.tensor(1, I32, 2); g.tensor(2, F32, 2); g.tensor(3, F32); g.optional(4, CNA_F64, 2); g.tensor(5, BF16, 4);
    g.scratch(6);
    if (int rc = g.rc()) return rc;
    const bool colour = g.given(4);
    const int64_t B = g.d(0, 0), Hs = g.d(0, 1), Ws = g.d(0, 2), Hp = g.d(5, 1), Wp = g.d(5, 2), C = g.d(5, 3);
    g.require(B >= 0 && Hs >= 0 && Ws >= 0 && g.d(0, 3) == 3 && g.d(1, 0) == B && g.d(1, 1) == 2 && g.d(2, 0) == B && g.d(2, 1) == 6);
    g.require(g.numel(3) == 6 && g.d(5, 0) == B && (C == 4 || C == 8));
    if (colour) g.require(g.d(4, 0) == B && g.d(4, 1) == 8);
    g.require(at->out_h >= 1 && at->out_w >= 1 && at->pad_lo >= 0 && at->pad_hi >= 0);
    g.require(Hp == (int64_t)at->out_h + at->pad_lo + at->pad_hi && Wp == (int64_t)at->out_w + at->pad_lo + at->pad_hi);
    if (int rc = g.rc()) return rc;
    const int64_t lim = (int64_t)1 << 30;
    if (B > CNA_MAX_BATCH || g.numel(0) >= lim || g.numel(5) >= lim) return MD_ERR_SIZE;
    if (g.given(6) && (uintptr_t)params[6] % 8 != 0) return MD_ERR_ARG;
    if (B == 0) return MD_OK;
    if (!g.have({0, 1, 2, 3, 5})) return MD_ERR_ARG;
    for (int k = 0; k < 5; ++k)
        if (params[k] && params[k] == params[5]) return MD_ERR_ARG;
    if (g.given(6) && params[6] == params[5]) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    ImageArgs a;
    a.Hs = (int)Hs; a.Ws = (int)Ws; a.Ho = at->out_h; a.Wo = at->out_w; a.Hp = (int)Hp; a.Wp = (int)Wp; a.C = (int)C; a.pad_lo = at->pad_lo;
    a.nblk = (int)(int64_t)cn_grey_chunks(a.Ho, a.Wo);
    a.img = (const uint8_t *)params[0]; a.sizes = (const int *)params[1]; a.mat = (const float *)params[2]; a.norm = (const float *)params[3];
    a.colour = colour ? (const double *)params[4] : nullptr; a.out = (uint16_t *)params[5];
    a.part = nullptr; a.mean = nullptr;
    const dim3 grid((unsigned)((Hp * Wp + 255) / 256), (unsigned)B);
    const int64_t need = md_cn_aug_image_workspace_bytes(B, a.Ho, a.Wo);
    Scratch ws;
    if (colour) {
        if (int rc = ws.acquire((size_t)need, g, 6, s)) return rc;
        a.part = (double *)ws.ptr; a.mean = a.part + (size_t)B * a.nblk;
        hipLaunchKernelGGL(cn_grey_kernel, dim3((unsigned)a.nblk, (unsigned)B), dim3(256), 0, s, a);
        hipLaunchKernelGGL(cn_grey_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, a);
        hipLaunchKernelGGL(cn_image_kernel<true>, grid, dim3(256), 0, s, a);
    } else {
        if (g.given(6) && g.workspace(6) >= 0 && g.workspace(6) < need) return MD_ERR_SIZE;   // (no scratch is taken without colour draws)
        hipLaunchKernelGGL(cn_image_kernel<false>, grid, dim3(256), 0, s, a);
    }
    return launched();
}
