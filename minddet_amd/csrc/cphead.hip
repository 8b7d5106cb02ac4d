// cphead.hip -- CenterPoint (CenterHead) post-processing for every task and sample of a batch (include/minddet_hip_cp.h), reference
// paths relative to minddet/models/centerpoint:
//   md_cp_scores           det3d_ms/models/bbox_heads/center_head.py:297-334 (predict), :408-423 (the score / range mask), every cell
//                          of every task in one pass over the head tensor
//   md_cp_decode_selected  center_head.py:310-334 on the selected cells only + :426-430 (the operand of the rotated NMS)
//   md_cp_pack             center_head.py:455-458 (count = min(num_out, mask_num, nms_post_max_size)) + tools_ms/eval.py:84-111 (the
//                          task merge)
// The rotated NMS between the last two is md_nms_rotated (nms.hip).  The per-cell arithmetic is box_codec.h's (cp_score_one,
// cp_box_one), the functions md_centerpoint_decode runs.  Plain kernels: next to the convs that produce the head tensor their
// traffic is nothing (nuScenes, B = 4: 9.4 MB read once, 1.6 MB of scores written).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "aot.h"
#include "device.h"
#include "box_codec.h"
#include "../../include/minddet_hip_cp.h"

#pragma clang fp contract(off)

// the layout the host mirrors are written against (tests/test_centerpoint_post_cpu.py parses the header to the same numbers)
static_assert(sizeof(md_cp_task_attrs) == 32 && sizeof(md_cp_head_attrs) == 312 && offsetof(md_cp_head_attrs, score_threshold) == 260 &&
                  offsetof(md_cp_head_attrs, max_per_task) == 308 && sizeof(md_nms_rotated_attrs) == 12,
              "minddet_hip_cp.h: attribute struct layout");

namespace md {

struct CpHead {
    CpTask task[MD_CP_MAX_TASKS];
    CpGeom g;
    int T, C, H, W;
};

constexpr int CPS_CELLS = 64;   // cells per workgroup of cp_scores_kernel

// 64 consecutive cells per workgroup: their C channels are staged through LDS with coalesced loads (rows padded by one dword so that
// the per-cell reads that follow spread over the banks), then lane = cell and the four waves share the tasks (wave w: tasks w, w + 4).
// The head tensor is read once for all tasks.  VEC: rows of C % 8 == 0 channels on a 16-byte aligned base -> 16-byte loads.
template <int VEC>
__global__ __launch_bounds__(256) void cp_scores_kernel(const uint16_t *__restrict__ head, CpHead a, long long cells_total,
                                                        float *__restrict__ scores) {
    extern __shared__ unsigned cps_sm[];
    const int rs = (a.C + 2) & ~1;   // halfwords per staged row (even, > C)
    const long long cell0 = (long long)blockIdx.x * CPS_CELLS;
    if (VEC) {
        const int chunks = a.C / 8;
        for (int i = threadIdx.x; i < CPS_CELLS * chunks; i += 256) {
            const int c = i / chunks, q = i - c * chunks;
            if (cell0 + c < cells_total) {
                const uint4 v = *reinterpret_cast<const uint4 *>(head + (size_t)(cell0 + c) * a.C + q * 8);
                unsigned *d = cps_sm + c * (rs / 2) + q * 4;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        }
    } else {
        uint16_t *sh = reinterpret_cast<uint16_t *>(cps_sm);
        for (int i = threadIdx.x; i < CPS_CELLS * a.C; i += 256) {
            const int c = i / a.C, q = i - c * a.C;
            if (cell0 + c < cells_total) sh[c * rs + q] = head[(size_t)(cell0 + c) * a.C + q];
        }
    }
    __syncthreads();
    const int c = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long cell = cell0 + c;
    if (cell >= cells_total) return;
    const int n = a.H * a.W;
    const long long b = cell / n;
    const int loc = (int)(cell - b * n);
    const int y = loc / a.W, x = loc - y * a.W;
    const uint16_t *h = reinterpret_cast<const uint16_t *>(cps_sm) + c * rs;
    for (int t = wave; t < a.T; t += 4) {
        int lab;
        float ctr[3];
        scores[((size_t)b * a.T + t) * n + loc] = cp_score_one(h, a.task[t], a.g, x, y, lab, ctr);
    }
}

__global__ __launch_bounds__(256) void cp_decode_selected_kernel(const uint16_t *__restrict__ head, CpHead a, int B, int k,
                                                                 const int *__restrict__ idx, const int *__restrict__ cnt,
                                                                 float *__restrict__ boxes, float *__restrict__ nms_boxes,
                                                                 int *__restrict__ labels) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;   // B T k < 2^31 / 9 (checked by the host)
    if (r >= B * a.T * k) return;
    const int bt = r / k, j = r - bt * k;
    const int b = bt / a.T, t = bt - b * a.T;
    float bb[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, nn[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int lab = 0;
    const int n = a.H * a.W;
    const int loc = j < cnt[bt] ? idx[r] : -1;
    if (loc >= 0 && loc < n) {
        const int y = loc / a.W, x = loc - y * a.W;
        const uint16_t *h = head + ((size_t)b * n + loc) * a.C;
        float ctr[3];
        (void)cp_score_one(h, a.task[t], a.g, x, y, lab, ctr);
        cp_box_one(h, a.task[t], ctr, bb, nn);
    }
    float *o = boxes + (size_t)r * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) o[q] = bb[q];
    float *on = nms_boxes + (size_t)r * 7;
#pragma unroll
    for (int q = 0; q < 7; ++q) on[q] = nn[q];
    labels[r] = lab;
}

struct CpPackArgs {
    const float *boxes, *sel_scores;
    const int *labels, *keep_idx, *num, *cnt;
    float *dets;
    int *count;
    int T, k, m;
    int class_base[MD_CP_MAX_TASKS];
};

// one workgroup per sample: the tasks' sizes (LDS counters), their prefix sum, then every element of the sample's dets rows
__global__ __launch_bounds__(256) void cp_pack_kernel(CpPackArgs a) {
    __shared__ int s_size[MD_CP_MAX_TASKS], s_base[MD_CP_MAX_TASKS + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < MD_CP_MAX_TASKS) s_size[tid] = 0;
    __syncthreads();
    const int rows = a.T * a.m;
    for (int e = tid; e < rows; e += 256) {
        const int t = e / a.m, j = e - t * a.m;
        const int bt = b * a.T + t;
        const int c = min(min(a.num[bt], a.cnt[bt]), min(a.m, a.k));
        if (j < c) {
            const int ki = a.keep_idx[(size_t)bt * a.k + j];
            if (ki >= 0 && ki < a.k && a.sel_scores[(size_t)bt * a.k + ki] > 0.f) atomicAdd(&s_size[t], 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        int base = 0;
        for (int t = 0; t < a.T; ++t) { s_base[t] = base; base += s_size[t]; }
        for (int t = a.T; t <= MD_CP_MAX_TASKS; ++t) s_base[t] = base;
        a.count[b] = base;
    }
    __syncthreads();
    const int total = s_base[a.T];
    float *out = a.dets + (size_t)b * rows * 11;
    for (int e = tid; e < rows * 11; e += 256) {
        const int r = e / 11, q = e - r * 11;
        float v = 0.f;
        if (r < total) {
            int t = 0;
            while (r >= s_base[t + 1]) ++t;   // t < T: r < total = s_base[T]
            const int bt = b * a.T + t;
            const int ki = a.keep_idx[(size_t)bt * a.k + (r - s_base[t])];
            if (ki >= 0 && ki < a.k) {
                const size_t row = (size_t)bt * a.k + ki;
                v = q < 9 ? a.boxes[row * 9 + q] : q == 9 ? a.sel_scores[row] : (float)(a.labels[row] + a.class_base[t]);
            }
        }
        out[e] = v;
    }
}

// the checks every head op shares: the attribute struct against the head tensor's channels; fills h
static int cp_head_of(const md_cp_head_attrs *at, int64_t H, int64_t W, int64_t C, CpHead &h) {
    if (at->num_tasks < 1 || at->num_tasks > MD_CP_MAX_TASKS || H < 0 || W < 0 || C < 0) return MD_ERR_ARG;
    for (int t = 0; t < at->num_tasks; ++t) {
        const md_cp_task_attrs &s = at->task[t];
        if (s.num_classes < 1 || s.off_hm < 0 || (int64_t)s.off_hm + s.num_classes > C || s.off_reg < 0 || (int64_t)s.off_reg + 2 > C ||
            s.off_height < 0 || (int64_t)s.off_height + 1 > C || s.off_dim < 0 || (int64_t)s.off_dim + 3 > C || s.off_rot < 0 ||
            (int64_t)s.off_rot + 2 > C || s.off_vel < -1 || (int64_t)s.off_vel + 2 > C)
            return MD_ERR_ARG;
        h.task[t] = {s.off_reg, s.off_height, s.off_dim, s.off_rot, s.off_vel, s.off_hm, s.num_classes};
    }
    for (int t = at->num_tasks; t < MD_CP_MAX_TASKS; ++t) h.task[t] = {0, 0, 0, 0, -1, 0, 0};
    if (H > 65536 || W > 65536) return MD_ERR_SIZE;
    h.g.score_thr = at->score_threshold; h.g.osf = at->out_size_factor; h.g.vx = at->voxel_size[0]; h.g.vy = at->voxel_size[1];
    h.g.px = at->pc_range[0]; h.g.py = at->pc_range[1];
    for (int i = 0; i < 3; ++i) { h.g.rmin[i] = at->post_center_range[i]; h.g.rmax[i] = at->post_center_range[3 + i]; }
    h.T = at->num_tasks; h.C = (int)C; h.H = (int)H; h.W = (int)W;
    return MD_OK;
}

}  // namespace md

using namespace md;

// in : head[B,H,W,C] bf16 ; out: scores[B,T,n] f32.  extra: md_cp_head_attrs (required).  Every check precedes the first device call.
extern "C" int md_cp_scores(MD_AOT_ARGS) {
    Args g(MD_ARGS, 2, 2);
    const md_cp_head_attrs *at = g.attrs<md_cp_head_attrs>(extra);
    g.tensor(0, BF16, 4); g.tensor(1, F32, 3);
    if (int rc = g.rc()) return rc;
    const int64_t B = g.d(0, 0), H = g.d(0, 1), W = g.d(0, 2), C = g.d(0, 3);
    CpHead h;
    if (B < 0) return MD_ERR_ARG;
    if (int rc = cp_head_of(at, H, W, C, h)) return rc;
    const int64_t n = H * W, T = h.T;
    if (g.d(1, 0) != B || g.d(1, 1) != T || g.d(1, 2) != n) return MD_ERR_ARG;
    if (C > 480 || !fits_i32(mul({B, T, n})) || !fits_i32(mul({B, n, C}))) return MD_ERR_SIZE;
    if (B * n == 0) return MD_OK;
    if (!g.have({0, 1})) return MD_ERR_ARG;
    const uint16_t *head = g.ptr<const uint16_t>(0);
    const bool vec = C % 8 == 0 && ((uintptr_t)head % 16) == 0;
    const size_t lds = (size_t)CPS_CELLS * ((C + 2) & ~1) * 2;
    const long long cells = B * n;
    hipLaunchKernelGGL(vec ? cp_scores_kernel<1> : cp_scores_kernel<0>, dim3((unsigned)((cells + CPS_CELLS - 1) / CPS_CELLS)), dim3(256),
                       lds, (hipStream_t)stream, head, h, cells, g.ptr<float>(1));
    return launched();
}

// in : head[B,H,W,C] bf16, idx[B,T,k] i32, cnt[B,T] i32 ; out: boxes[B,T,k,9] f32, nms_boxes[B,T,k,7] f32, labels[B,T,k] i32.
// extra: md_cp_head_attrs (required)
extern "C" int md_cp_decode_selected(MD_AOT_ARGS) {
    Args g(MD_ARGS, 6, 6);
    const md_cp_head_attrs *at = g.attrs<md_cp_head_attrs>(extra);
    g.tensor(0, BF16, 4); g.tensor(1, I32, 3); g.tensor(2, I32, 2); g.tensor(3, F32, 4); g.tensor(4, F32, 4); g.tensor(5, I32, 3);
    if (int rc = g.rc()) return rc;
    const int64_t B = g.d(0, 0), H = g.d(0, 1), W = g.d(0, 2), C = g.d(0, 3), k = g.d(1, 2);
    CpHead h;
    if (B < 0 || k < 0) return MD_ERR_ARG;
    if (int rc = cp_head_of(at, H, W, C, h)) return rc;
    const int64_t T = h.T;
    if (g.d(1, 0) != B || g.d(1, 1) != T || g.d(2, 0) != B || g.d(2, 1) != T) return MD_ERR_ARG;
    if (g.d(3, 0) != B || g.d(3, 1) != T || g.d(3, 2) != k || g.d(3, 3) != 9 || g.d(4, 0) != B || g.d(4, 1) != T || g.d(4, 2) != k ||
        g.d(4, 3) != 7 || g.d(5, 0) != B || g.d(5, 1) != T || g.d(5, 2) != k)
        return MD_ERR_ARG;
    if (!fits_i32(mul({B, T, k, 9})) || !fits_i32(mul({B, H, W, C}))) return MD_ERR_SIZE;
    if (B * k == 0) return MD_OK;
    if (!g.have({0, 1, 2, 3, 4, 5})) return MD_ERR_ARG;
    hipLaunchKernelGGL(cp_decode_selected_kernel, dim3((unsigned)((B * T * k + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       g.ptr<const uint16_t>(0), h, (int)B, (int)k, g.ptr<const int>(1), g.ptr<const int>(2), g.ptr<float>(3),
                       g.ptr<float>(4), g.ptr<int>(5));
    return launched();
}

// in : boxes[B,T,k,9] f32, sel_scores[B,T,k] f32, labels[B,T,k] i32, keep_idx[B,T,k] i32, num[B,T] i32, cnt[B,T] i32 ;
// out: dets[B,T m,11] f32, count[B] i32.  extra: md_cp_head_attrs (required)
extern "C" int md_cp_pack(MD_AOT_ARGS) {
    Args g(MD_ARGS, 8, 8);
    const md_cp_head_attrs *at = g.attrs<md_cp_head_attrs>(extra);
    g.tensor(0, F32, 4); g.tensor(1, F32, 3); g.tensor(2, I32, 3); g.tensor(3, I32, 3); g.tensor(4, I32, 2); g.tensor(5, I32, 2);
    g.tensor(6, F32, 3); g.tensor(7, I32, 1);
    if (int rc = g.rc()) return rc;
    const int64_t B = g.d(0, 0), T = g.d(0, 1), k = g.d(0, 2), m = at->max_per_task;
    if (at->num_tasks < 1 || at->num_tasks > MD_CP_MAX_TASKS || at->num_tasks != T || m < 0 || B < 0 || k < 0 || g.d(0, 3) != 9)
        return MD_ERR_ARG;
    for (int i = 1; i <= 3; ++i)
        if (g.d(i, 0) != B || g.d(i, 1) != T || g.d(i, 2) != k) return MD_ERR_ARG;
    for (int i = 4; i <= 5; ++i)
        if (g.d(i, 0) != B || g.d(i, 1) != T) return MD_ERR_ARG;
    if (g.d(6, 0) != B || g.d(6, 1) != T * m || g.d(6, 2) != 11 || g.d(7, 0) != B) return MD_ERR_ARG;
    if (mul({T, m}) > 65536 || !fits_i32(mul({B, T, k, 9})) || !fits_i32(mul({B, T, m, 11}))) return MD_ERR_SIZE;
    if (B == 0) return MD_OK;
    if (!g.have({6, 7}) || (k > 0 && !g.have({0, 1, 2, 3})) || !g.have({4, 5})) return MD_ERR_ARG;
    CpPackArgs a;
    a.boxes = g.ptr<const float>(0); a.sel_scores = g.ptr<const float>(1); a.labels = g.ptr<const int>(2);
    a.keep_idx = g.ptr<const int>(3); a.num = g.ptr<const int>(4); a.cnt = g.ptr<const int>(5);
    a.dets = g.ptr<float>(6); a.count = g.ptr<int>(7);
    a.T = (int)T; a.k = (int)k; a.m = (int)m;
    for (int t = 0; t < MD_CP_MAX_TASKS; ++t) a.class_base[t] = t < T ? at->task[t].class_base : 0;
    hipLaunchKernelGGL(cp_pack_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    return launched();
}
