// loss_common.h -- what the training losses (cploss.hip, pploss.hip, cnloss.hip) share, stated once: the fixed-order block sums, the
// CenterNet-style focal terms, the strip staging of the dense kernels, the L1 slot pieces and the host-side rules of the entries.
// The losses promise bit-equal results from call to call: the summation order that promise rests on is block_sums below.
// Pieces only: each loss keeps its Params struct, its kernels, its argument checks and its error codes.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "aot.h"
#include "device.h"
#include "workgroup.h"

#pragma clang fp contract(off)

namespace md {

// ---------------------------------------------------------------------------------------------------- block reductions
// N block sums at once, in a fixed order (256 lanes; red: 4 N doubles); every lane gets the sums
template <int N> __device__ __forceinline__ void block_sums(double (&v)[N], double *red) {
#pragma unroll
    for (int e = 0; e < N; ++e)
        for (int off = 32; off > 0; off >>= 1) v[e] += __shfl_down(v[e], off, 64);
    __syncthreads();   // red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int e = 0; e < N; ++e) red[(threadIdx.x >> 6) * N + e] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = ((red[e] + red[N + e]) + red[2 * N + e]) + red[3 * N + e];
}
// (block_count, the block sum of integers: workgroup.h)

// ---------------------------------------------------------------------------------------------------- focal terms (CenterNet form)
// A term and its derivative are two functions (the logs and squares they both spell are computed once after inlining): a caller that
// wants one alone says so, and cn_loss_dense_kernel adds the term to its sum before it forms the derivative -- with both handed back by
// one call the compiler merged the two sums' additions behind the branch into selects, 5 % on that kernel.
// p = clip(sigmoid(x), 1e-4, 1 - 1e-4); open: the clip passes the gradient
__device__ __forceinline__ double clipped_p(float x, bool &open) {
    const double s = 1.0 / (1.0 + exp(-(double)x));
    open = s > 1e-4 && s < 1.0 - 1e-4;
    return fmin(fmax(s, 1e-4), 1.0 - 1e-4);
}
// the negative focal term log(1 - p) p^2 (1 - hm)^4, and its derivative with respect to the logit (0 where the clip is active)
__device__ __forceinline__ double neg_term(double p, float hmv) {
    const double q = 1.0 - (double)hmv, q2 = q * q, g4 = q2 * q2;
    const double l1p = log(1.0 - p);
    return l1p * (p * p) * g4;
}
__device__ __forceinline__ double neg_term_grad(double p, bool open, float hmv) {
    const double q = 1.0 - (double)hmv, q2 = q * q, g4 = q2 * q2;
    const double l1p = log(1.0 - p);
    return open ? g4 * (p * p) * (2.0 * (1.0 - p) * l1p - p) : 0.0;
}
// the positive focal term log(p) (1 - p)^2, and its derivative with respect to the logit
__device__ __forceinline__ double pos_term(double p) {
    const double lp = log(p), om = 1.0 - p;
    return lp * (om * om);
}
__device__ __forceinline__ double pos_term_grad(double p, bool open) {
    const double lp = log(p), om = 1.0 - p;
    return open ? (om * om) * (om - 2.0 * p * lp) : 0.0;
}

// ---------------------------------------------------------------------------------------------------- L1 slots
__device__ __forceinline__ bool slot_valid(int m, int i, int HW) { return m != 0 && i >= 0 && i < HW; }
__device__ __forceinline__ int l1_sign(float pred, float target) { return (pred > target) - (pred < target); }
// weight sgn / den rounded once; +0 when the signs cancel, whatever the weight's sign
__device__ __forceinline__ float reg_grad(float weight, int sgn, double den) { return sgn == 0 ? 0.f : (float)((double)weight * (double)sgn / den); }

// ---------------------------------------------------------------------------------------------------- strips of the dense kernels
// A dense kernel's workgroup owns `strip` consecutive cells of one sample, all C channels of them: elems elements from `base` on, in
// head (bf16, staged in LDS) and in grad (fp32, assembled in LDS and stored once).
struct Strip {
    int b, n0, cells, elems;   // sample, first cell, cells (fewer in a sample's last strip), cells C
    size_t base;
};
__device__ __forceinline__ Strip strip_of_block(int strips_per_sample, int strip, int HW, int C) {
    const int b = blockIdx.x / strips_per_sample, n0 = (blockIdx.x - b * strips_per_sample) * strip;
    const int cells = min(strip, HW - n0);
    return {b, n0, cells, cells * C, ((size_t)b * HW + n0) * C};
}
// vec (strip_vec below): every strip starts on a 16-byte boundary in head and in grad and holds a multiple of 8 elements
// the strip's head rows into sh; with GRAD the grad strip sg cleared (256 lanes; the caller's next barrier publishes both)
template <bool GRAD>
__device__ __forceinline__ void stage_strip(uint16_t *sh, float *sg, const uint16_t *__restrict__ src, int elems, int vec) {
    if (vec) {
        for (int i = threadIdx.x; i < elems / 8; i += 256) ((uint4 *)sh)[i] = ((const uint4 *)src)[i];
        if (GRAD)
            for (int i = threadIdx.x; i < elems / 4; i += 256) ((float4 *)sg)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (int i = threadIdx.x; i < elems; i += 256) sh[i] = src[i];
        if (GRAD)
            for (int i = threadIdx.x; i < elems; i += 256) sg[i] = 0.f;
    }
}
// the grad strip to memory, contiguously (a barrier stands between the last write of sg and this call)
__device__ __forceinline__ void flush_strip(float *__restrict__ dst, const float *sg, int elems, int vec) {
    if (vec) {
        for (int i = threadIdx.x; i < elems / 4; i += 256) ((float4 *)dst)[i] = ((const float4 *)sg)[i];
    } else {
        for (int i = threadIdx.x; i < elems; i += 256) dst[i] = sg[i];
    }
}

// ---------------------------------------------------------------------------------------------------- host side of the entries
// each gradient element has one owner: the n heads' channel ranges [lo, hi) inside [0, C) and pairwise apart
static inline void heads_disjoint(Args &a, const int64_t *lo, const int64_t *hi, int n, int64_t C) {
    for (int i = 0; i < n; ++i) {
        a.require(lo[i] >= 0 && hi[i] <= C);
        for (int j = i + 1; j < n; ++j) a.require(hi[i] <= lo[j] || hi[j] <= lo[i]);
    }
}
// the 16-byte path of stage_strip / flush_strip: `period` (elements; every strip's start and length are multiples of it or of
// 64 C) a multiple of 8 and both pointers 16-byte aligned (grad NULL, the forward alone, counts as aligned)
static inline int strip_vec(int64_t period, const void *head, const void *grad) {
    return period % 8 == 0 && (uintptr_t)head % 16 == 0 && (uintptr_t)grad % 16 == 0;
}
// dynamic LDS of a dense kernel: its own words in front, then per cell `cell_bytes` of its own, the C bf16 head values and, with the
// gradient, C fp32
static inline size_t strip_lds_bytes(int lds_head, int strip, int64_t C, bool with_grad, int64_t cell_bytes = 0) {
    return lds_head + (size_t)strip * (cell_bytes + C * (with_grad ? 6 : 2));
}
// f(std::true_type) or f(std::false_type): an entry states the launches of its <GRAD> kernels once, in a generic lambda
template <typename F> static inline void grad_or_not(bool with_grad, F &&f) {
    if (with_grad) f(std::true_type{});
    else f(std::false_type{});
}

}  // namespace md
