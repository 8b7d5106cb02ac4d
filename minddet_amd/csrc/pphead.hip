// pphead.hip -- head post-processing of the anchor-based (KITTI) PointPillars (include/minddet_hip_pp.h), reference paths relative
// to minddet/models/pointpillars/src:
//   md_pp_scores           pointpillars.py:741-763 (get_total_scores, get_selected_data up to the mask), every anchor of the batch
//   md_pp_decode_selected  pointpillars.py:623-652 (generate_predicted_boxes) on the selected anchors only + predict.py:222-236 (the
//                          direction fix) + predict.py:61-78 (the standup boxes the NMS takes)
// Both read the merged head tensor [B,H,W,C] bf16 in place.  Plain kernels, lane = anchor / selected row: next to the convs that
// produce the head tensor their traffic is nothing (Car, B = 4: 20 MB read, 3.4 MB written).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aot.h"
#include "device.h"
#include "box_codec.h"
#include "../../include/minddet_hip_pp.h"

#pragma clang fp contract(off)

namespace md {

struct PPScoreArgs {
    const uint16_t *head;
    const unsigned char *mask;   // or nullptr
    float *scores;
    int *labels;
    size_t total;                // B * N
    int N, A, K, C, off_cls;
};

// running (maximum, first index that attains it) over the classes in order
#define PP_TAKE(BITS, KI)                              \
    do {                                               \
        const float s__ = sigmoid(bf2f(BITS));         \
        if ((KI) == 0 || s__ > best) { best = s__; lab = (KI); } \
    } while (0)

// VEC = the K class logits of an anchor as one load of 2 K bytes (K = 1 or 2, the KITTI models; an alignment the host has checked);
// VEC = 0: K scalar loads, any K
template <int VEC>
__global__ __launch_bounds__(256) void pp_scores_kernel(PPScoreArgs g) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < g.total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t b = e / (size_t)g.N;
        const int n = (int)(e - b * (size_t)g.N);
        const int cell = n / g.A, a = n - cell * g.A;
        const uint16_t *p = g.head + (b * (size_t)(g.N / g.A) + (size_t)cell) * (size_t)g.C + g.off_cls + a * g.K;
        float best = 0.f;
        int lab = 0;
        if (VEC == 1) {
            PP_TAKE(*p, 0);
        } else if (VEC == 2) {
            const uint32_t v = *reinterpret_cast<const uint32_t *>(p);
            PP_TAKE(v & 0xffffu, 0); PP_TAKE(v >> 16, 1);
        } else {
            for (int k = 0; k < g.K; ++k) PP_TAKE(p[k], k);
        }
        if (g.mask && g.mask[e] == 0) best = -1.0f;
        g.scores[e] = best;
        g.labels[e] = lab;
    }
}

struct PPDecodeArgs {
    const uint16_t *head;
    const float *anchors;
    const int *idx, *cnt;
    const float *sel_scores;
    const int *labels;
    float *dets, *standup, *boxes;   // boxes: or nullptr
    int *dir_labels;
    int B, k, N, A, C, off_box, off_dir;
};

__global__ __launch_bounds__(256) void pp_decode_selected_kernel(PPDecodeArgs g) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;   // B * k < 2^31 / 9 (checked by the host)
    if (r >= g.B * g.k) return;
    const int b = r / g.k, j = r - b * g.k;
    float d[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, raw[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
    int dir = 0;
    const int n = j < g.cnt[b] ? g.idx[r] : -1;
    if (n >= 0 && n < g.N) {
        const int cell = n / g.A, a = n - cell * g.A;
        const uint16_t *p = g.head + ((size_t)b * (size_t)(g.N / g.A) + (size_t)cell) * (size_t)g.C;
        float t[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) t[q] = bf2f(p[g.off_box + a * 7 + q]);
        second_box_decode_one(t, g.anchors + (size_t)n * 7, raw);
        st = standup_one(raw[0], raw[1], raw[3], raw[4], raw[6]);
        float rot = raw[6];
        if (g.off_dir >= 0) {
            const float d0 = bf2f(p[g.off_dir + a * 2]), d1 = bf2f(p[g.off_dir + a * 2 + 1]);
            dir = d1 > d0 ? 1 : 0;
            if ((rot > 0.f) != (dir != 0)) rot = rot + 3.14159265358979323846f;
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) d[q] = raw[q];
        d[6] = rot;
        d[7] = g.sel_scores[r];
        d[8] = (float)g.labels[(size_t)b * (size_t)g.N + (size_t)n];
    }
    float *o = g.dets + (size_t)r * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) o[q] = d[q];
    *reinterpret_cast<float4 *>(g.standup + (size_t)r * 4) = st;
    g.dir_labels[r] = dir;
    if (g.boxes) {
        float *ob = g.boxes + (size_t)r * 7;
#pragma unroll
        for (int q = 0; q < 7; ++q) ob[q] = raw[q];
    }
}

}  // namespace md

using namespace md;

// in : head[B,H,W,C] bf16, mask[B,N] u8 or NULL ; out: scores[B,N] f32, labels[B,N] i32.  extra: md_pp_head_attrs (required).
// Every check precedes the first device call.
extern "C" int md_pp_scores(MD_AOT_ARGS) {
    Args g(MD_ARGS, 4, 4);
    const md_pp_head_attrs *at = g.attrs<md_pp_head_attrs>(extra);
    g.tensor(0, BF16, 4); g.optional(1, U8, 2); g.tensor(2, F32, 2); g.tensor(3, I32, 2);
    if (int rc = g.rc()) return rc;
    const int64_t B = g.d(0, 0), H = g.d(0, 1), W = g.d(0, 2), C = g.d(0, 3);
    const int64_t A = at->num_anchors, K = at->num_classes;
    if (A <= 0 || K <= 0 || at->score_mode != 0 || B < 0 || H < 0 || W < 0 || C < 0) return MD_ERR_ARG;
    if (at->off_cls < 0 || at->off_cls + A * K > C) return MD_ERR_ARG;
    if (H > 65536 || W > 65536 || A > 65536) return MD_ERR_SIZE;
    const int64_t N = H * W * A;
    if (g.d(2, 0) != B || g.d(2, 1) != N || g.d(3, 0) != B || g.d(3, 1) != N) return MD_ERR_ARG;
    if (g.given(1) && (g.d(1, 0) != B || g.d(1, 1) != N)) return MD_ERR_ARG;
    if (!fits_i32(N) || !fits_i32(mul({B, N})) || !fits_i32(mul({B, H, W, C}))) return MD_ERR_SIZE;
    if (B * N == 0) return MD_OK;
    if (!g.have({0, 2, 3})) return MD_ERR_ARG;
    PPScoreArgs a;
    a.head = g.ptr<const uint16_t>(0); a.mask = g.given(1) ? g.ptr<const unsigned char>(1) : nullptr;
    a.scores = g.ptr<float>(2); a.labels = g.ptr<int>(3);
    a.total = (size_t)(B * N); a.N = (int)N; a.A = (int)A; a.K = (int)K; a.C = (int)C; a.off_cls = at->off_cls;
    // one load of 2 K bytes per lane needs the anchor's first logit on a 2 K byte boundary: the tensor base (the allocator's), every
    // cell's row (C) and the head's offset (off_cls) all multiples of K elements
    const bool vec = (K == 1 || K == 2) && C % K == 0 && at->off_cls % K == 0 && ((uintptr_t)a.head % (2 * K)) == 0;
    void (*k)(PPScoreArgs) = !vec ? pp_scores_kernel<0> : K == 1 ? pp_scores_kernel<1> : pp_scores_kernel<2>;
    hipLaunchKernelGGL(k, dim3(grid1d(a.total)), dim3(256), 0, (hipStream_t)stream, a);
    return launched();
}

// in : head[B,H,W,C] bf16, anchors[N,7] f32, idx[B,k] i32, cnt[B] i32, sel_scores[B,k] f32, labels[B,N] i32 ;
// out: dets[B,k,9] f32, standup[B,k,4] f32, dir_labels[B,k] i32 [, boxes[B,k,7] f32 or NULL].  extra: md_pp_head_attrs (required).
extern "C" int md_pp_decode_selected(MD_AOT_ARGS) {
    Args g(MD_ARGS, 9, 10);
    const md_pp_head_attrs *at = g.attrs<md_pp_head_attrs>(extra);
    g.tensor(0, BF16, 4); g.tensor(1, F32, 2); g.tensor(2, I32, 2); g.tensor(3, I32, 1); g.tensor(4, F32, 2); g.tensor(5, I32, 2);
    g.tensor(6, F32, 3); g.tensor(7, F32, 3); g.tensor(8, I32, 2); g.optional(9, F32, 3);
    if (int rc = g.rc()) return rc;
    const int64_t B = g.d(0, 0), H = g.d(0, 1), W = g.d(0, 2), C = g.d(0, 3), k = g.d(2, 1);
    const int64_t A = at->num_anchors;
    if (A <= 0 || at->self_train != 1 || B < 0 || H < 0 || W < 0 || C < 0 || k < 0) return MD_ERR_ARG;
    if (at->off_box < 0 || at->off_box + 7 * A > C || at->off_dir < -1 || (at->off_dir >= 0 && at->off_dir + 2 * A > C)) return MD_ERR_ARG;
    if (H > 65536 || W > 65536 || A > 65536) return MD_ERR_SIZE;
    const int64_t N = H * W * A;
    if (g.d(1, 0) != N || g.d(1, 1) != 7 || g.d(2, 0) != B || g.d(3, 0) != B || g.d(4, 0) != B || g.d(4, 1) != k || g.d(5, 0) != B ||
        g.d(5, 1) != N)
        return MD_ERR_ARG;
    if (g.d(6, 0) != B || g.d(6, 1) != k || g.d(6, 2) != 9 || g.d(7, 0) != B || g.d(7, 1) != k || g.d(7, 2) != 4 || g.d(8, 0) != B ||
        g.d(8, 1) != k)
        return MD_ERR_ARG;
    if (g.given(9) && (g.d(9, 0) != B || g.d(9, 1) != k || g.d(9, 2) != 7)) return MD_ERR_ARG;
    if (!fits_i32(mul({N, 7})) || !fits_i32(mul({B, N})) || !fits_i32(mul({B, k, 9})) || !fits_i32(mul({B, H, W, C}))) return MD_ERR_SIZE;
    if (B * k == 0) return MD_OK;
    if (!g.have({0, 1, 2, 3, 4, 5, 6, 7, 8})) return MD_ERR_ARG;
    PPDecodeArgs a;
    a.head = g.ptr<const uint16_t>(0); a.anchors = g.ptr<const float>(1); a.idx = g.ptr<const int>(2); a.cnt = g.ptr<const int>(3);
    a.sel_scores = g.ptr<const float>(4); a.labels = g.ptr<const int>(5);
    a.dets = g.ptr<float>(6); a.standup = g.ptr<float>(7); a.dir_labels = g.ptr<int>(8);
    a.boxes = g.given(9) ? g.ptr<float>(9) : nullptr;
    a.B = (int)B; a.k = (int)k; a.N = (int)N; a.A = (int)A; a.C = (int)C; a.off_box = at->off_box; a.off_dir = at->off_dir;
    hipLaunchKernelGGL(pp_decode_selected_kernel, dim3((unsigned)((B * k + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launched();
}
