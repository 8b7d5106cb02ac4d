// optim.hip -- the optimizer step on the device (include/minddet_hip_train.h): md_grad_sumsq, the squared norm of a flat gradient in
// float64 in a fixed order, and md_adam_step, Adam.construct of the reference (minddet/models/centerpoint/det3d_ms/solver/
// custom_adam.py:590-668: global-norm clip, decay_weight, scale_grad, then the dense update of :188-222) for one flat fp32 range in one
// launch, with the bf16 copy of the new weights the convs read written in the same pass.
//   grad_sumsq_kernel         one workgroup per chunk of 4096 elements (every 1024th chunk beyond 1024 workgroups): a float64 partial
//   grad_sumsq_finish_kernel  one workgroup over the partials
//   adam_step_kernel          four elements per lane by 16-byte loads and stores where the four tensors allow it, a scalar tail
// Arithmetic: float64 from the fp32 operands, each state rounded once (the header says why).  The order of the sums: block_sums.
#include "loss_common.h"
#include "../../include/minddet_hip_train.h"

#pragma clang fp contract(off)

namespace md {

static_assert(sizeof(md_adam_attrs) == 10 * 8, "minddet_hip_train.h: attribute struct layout");

constexpr int GS_CHUNK = MD_GRAD_SUMSQ_CHUNK;
constexpr int GS_MAX_BLOCKS = MD_GRAD_SUMSQ_MAX_BLOCKS;

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float *__restrict__ g, long long n, long long chunks, double *__restrict__ part) {
    __shared__ double red[4];
    double acc[1] = {0.0};
    for (long long c = blockIdx.x; c < chunks; c += GS_MAX_BLOCKS) {
        const long long base = c * GS_CHUNK;
        const int m = (int)min((long long)GS_CHUNK, n - base);
        for (int i = threadIdx.x; i < m; i += 256) {
            const double v = (double)g[base + i];
            acc[0] += v * v;
        }
    }
    block_sums<1>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(256) void grad_sumsq_finish_kernel(const double *__restrict__ part, int nb, double *__restrict__ out) {
    __shared__ double red[4];
    double acc[1] = {0.0};
    for (int i = threadIdx.x; i < nb; i += 256) acc[0] += part[i];
    block_sums<1>(acc, red);
    if (threadIdx.x == 0) out[0] = acc[0];
}

struct AdamParams {
    double lr_t, beta1, beta2, eps, weight_decay, max_norm, grad_scale;
    long long n, ns;
    int K, vec;   // vec: grad, param, m, v are 16-byte aligned (shadow: 8-byte, or absent)
};

struct AdamOut { float p, m, v; };
__device__ __forceinline__ AdamOut adam_element(float gf, float pf, float mf, float vf, const AdamParams &a, bool clip, double coef) {
    double g = (double)gf;
    const double p = (double)pf;
    if (clip) g = g * coef;
    g = g + a.weight_decay * p;
    g = g * a.grad_scale;
    const double m = a.beta1 * (double)mf + (1.0 - a.beta1) * g;
    const double v = a.beta2 * (double)vf + (1.0 - a.beta2) * (g * g);
    const double np = p - a.lr_t * (m / (sqrt(v) + a.eps));
    return {(float)np, (float)m, (float)v};
}

__global__ __launch_bounds__(256) void adam_step_kernel(const float *__restrict__ grad, const double *__restrict__ sumsq, float *__restrict__ param,
                                                        float *__restrict__ m, float *__restrict__ v, uint16_t *__restrict__ shadow, AdamParams a) {
    bool clip = false;
    double coef = 1.0;
    if (sumsq) {   // every lane forms the same coefficient from the same K values in the same order
        double t = 0.0;
        for (int k = 0; k < a.K; ++k) t += sumsq[k];
        coef = a.max_norm / (sqrt(t) + 1e-6);
        clip = coef < 1.0;
    }
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nthreads = (long long)gridDim.x * 256;
    const long long nvec = a.vec ? a.n / 4 : 0;
    for (long long i = tid; i < nvec; i += nthreads) {
        const f32x4 g4 = ((const f32x4 *)grad)[i];
        f32x4 p4 = ((f32x4 *)param)[i], m4 = ((f32x4 *)m)[i], v4 = ((f32x4 *)v)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const AdamOut o = adam_element(g4[e], p4[e], m4[e], v4[e], a, clip, coef);
            p4[e] = o.p; m4[e] = o.m; v4[e] = o.v;
        }
        ((f32x4 *)param)[i] = p4;
        ((f32x4 *)m)[i] = m4;
        ((f32x4 *)v)[i] = v4;
        const long long e0 = 4 * i;
        if (e0 + 4 <= a.ns) {
            ((u32x2 *)shadow)[i] = (u32x2){(unsigned)f2bf(p4[0]) | ((unsigned)f2bf(p4[1]) << 16), (unsigned)f2bf(p4[2]) | ((unsigned)f2bf(p4[3]) << 16)};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e0 + e < a.ns) shadow[e0 + e] = f2bf(p4[e]);
        }
    }
    for (long long i = 4 * nvec + tid; i < a.n; i += nthreads) {   // the tail, or everything where a tensor is not aligned
        const AdamOut o = adam_element(grad[i], param[i], m[i], v[i], a, clip, coef);
        param[i] = o.p;
        m[i] = o.m;
        v[i] = o.v;
        if (i < a.ns) shadow[i] = f2bf(o.p);
    }
}

static int64_t grad_sumsq_blocks(int64_t n) {
    const int64_t chunks = n / GS_CHUNK + (n % GS_CHUNK != 0);
    return chunks < 1 ? 1 : (chunks > GS_MAX_BLOCKS ? GS_MAX_BLOCKS : chunks);
}

static int grad_sumsq_entry(MD_AOT_ARGS) {
    // in : grad[n] f32 ; out: sumsq[1] f64 ; [workspace]
    const int WS = 2;
    Args a(MD_ARGS, WS, WS + 1);
    a.tensor(0, F32, 1); a.tensor(1, "float64", 1);
    a.scratch(WS);
    if (int rc = a.rc()) return rc;
    const int64_t n = a.d(0, 0);
    a.require(n >= 1 && a.d(1, 0) == 1);
    if (int rc = a.rc()) return rc;
    if (n >= ((int64_t)1 << 31)) return MD_ERR_SIZE;
    if (!a.have({0, 1})) return MD_ERR_ARG;
    const int64_t nb = grad_sumsq_blocks(n);
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = acquire_aligned(ws, (size_t)(8 * nb), a, WS, s, 8)) return rc;
    double *part = (double *)ws.ptr;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const float *)params[0], (long long)n,
                       (long long)((n + GS_CHUNK - 1) / GS_CHUNK), part);
    hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(256), 0, s, part, (int)nb, (double *)params[1]);
    return launched();
}

static int adam_step_entry(MD_AOT_ARGS) {
    // in : grad[n] f32, sumsq[K] f64 or NULL ; in / out: param[n], m[n], v[n] f32 ; out: shadow[ns] bf16 or NULL
    Args a(MD_ARGS, 6, 6);
    const md_adam_attrs *at = a.attrs<md_adam_attrs>(extra);
    a.tensor(0, F32, 1); a.optional(1, "float64", 1); a.tensor(2, F32, 1); a.tensor(3, F32, 1); a.tensor(4, F32, 1); a.optional(5, BF16, 1);
    if (int rc = a.rc()) return rc;
    const int64_t n = a.d(0, 0);
    const bool clip = a.given(1), with_shadow = a.given(5);
    const int64_t K = clip ? a.d(1, 0) : 0, ns = with_shadow ? a.d(5, 0) : 0;
    a.require(n >= 1 && a.d(2, 0) == n && a.d(3, 0) == n && a.d(4, 0) == n && ns <= n && (!clip || K >= 1));
    const double fl[] = {at->lr, at->beta1, at->beta2, at->beta1_power, at->beta2_power, at->eps, at->weight_decay, at->max_norm, at->grad_scale,
                         at->reserved0};
    for (double v : fl) a.require(isfinite(v));
    a.require(at->reserved0 == 0.0 && at->lr >= 0.0 && at->beta1 >= 0.0 && at->beta1 < 1.0 && at->beta2 >= 0.0 && at->beta2 < 1.0);
    a.require(at->beta1_power >= 0.0 && at->beta1_power < 1.0 && at->beta2_power >= 0.0 && at->beta2_power < 1.0);
    a.require(at->eps >= 0.0 && at->grad_scale >= 0.0 && (!clip || at->max_norm > 0.0));
    a.require(!aliased(params, 2, 6));
    if (int rc = a.rc()) return rc;
    if (n >= ((int64_t)1 << 31) || K > MD_ADAM_MAX_SUMSQ) return MD_ERR_SIZE;
    if (!a.have({0, 2, 3, 4})) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;

    AdamParams p;
    memset(&p, 0, sizeof(p));
    p.lr_t = at->lr * sqrt(1.0 - at->beta2_power) / (1.0 - at->beta1_power);
    p.beta1 = at->beta1; p.beta2 = at->beta2; p.eps = at->eps; p.weight_decay = at->weight_decay; p.max_norm = at->max_norm;
    p.grad_scale = at->grad_scale;
    p.n = n; p.ns = ns; p.K = (int)K;
    p.vec = ((uintptr_t)params[0] | (uintptr_t)params[2] | (uintptr_t)params[3] | (uintptr_t)params[4]) % 16 == 0 &&
            (!with_shadow || (uintptr_t)params[5] % 8 == 0);
    hipLaunchKernelGGL(adam_step_kernel, dim3(grid1d((size_t)(n + 3) / 4, 4096)), dim3(256), 0, s, (const float *)params[0],
                       clip ? (const double *)params[1] : nullptr, (float *)params[2], (float *)params[3], (float *)params[4],
                       with_shadow ? (uint16_t *)params[5] : nullptr, p);
    return launched();
}

}  // namespace md

using namespace md;

extern "C" int64_t md_grad_sumsq_workspace_bytes(int64_t n) { return any_negative({n}) ? -1 : 8 * grad_sumsq_blocks(n); }
extern "C" int md_grad_sumsq(MD_AOT_ARGS) { return grad_sumsq_entry(nparam, params, ndims, shapes, dtypes, stream, extra); }
extern "C" int md_adam_step(MD_AOT_ARGS) { return adam_step_entry(nparam, params, ndims, shapes, dtypes, stream, extra); }
