// cptargets.hip -- CenterPoint training targets on the device (include/minddet_hip_cptargets.h; the consumer-side twin of cphead.hip).
//
// What it replaces: AssignLabel.__call__ (minddet/models/centerpoint/det3d_ms/datasets/pipelines/preprocess.py:297-521) with
// gaussian_radius / gaussian2D / draw_umich_gaussian (det3d_ms/core/utils/center_utils.py:16-65) and limit_period
// (det3d_ms/core/bbox/box_np_ops.py:247-248): a Python loop per object with a numpy window maximum per Gaussian, on the host.
// Two launches and no host read:
//   cp_slot_kernel  one workgroup per (sample, task): the sample's rows staged in LDS, membership and slot ranks by counting, every row
//                   of ind / mask / cat / anno_box and the task's rows of gt_boxes_and_cls written once, and the task's draw list
//                   (ct_int x, y, radius, class; one entry per slot, radius -1 for a skipped row) left in the workspace
//   cp_heat_kernel  heatmap.h's heat_tile on one 64 x 16 tile of one (sample, task, class) map, the task's draw list filtered by class
// Same float32 operation order as the numpy code under NumPy >= 2 scalar promotion (fp contraction off); the Gaussian in float64.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "aot.h"
#include "../../include/minddet_hip_cptargets.h"

#pragma clang fp contract(off)

#include "heatmap.h"

namespace md {

static_assert(sizeof(md_cp_targets_attrs) == 4 + 8 * 4 + 2 * 4 + 2 * 4 + 4 + 4 + 4, "minddet_hip_cptargets.h: attribute struct layout");

constexpr int CPT_MAX_GT = MD_CP_TARGETS_MAX_GT;
constexpr int CPT_INVALID = 0x7fffffff;

struct CptParams {
    int G, M, T, C, H, W;
    int total_classes;
    int class_base[MD_CP_TARGETS_MAX_TASKS], num_classes[MD_CP_TARGETS_MAX_TASKS];
    float vs_x, vs_y, pc_x, pc_y, osf, overlap;
    int min_radius;
};

// gaussian_radius((height, width) = (l, w), overlap), center_utils.py:16-36 term by term in fp32
__device__ __forceinline__ float gaussian_radius_f32(float height, float width, float o) {
    const float om = 1.f - o, op = 1.f + o;
    const float b1 = height + width;
    const float c1 = width * height * om / op;
    const float sq1 = sqrtf(b1 * b1 - 4.f * c1);
    const float r1 = (b1 + sq1) / 2.f;
    const float b2 = 2.f * (height + width);
    const float c2 = om * width * height;
    const float sq2 = sqrtf(b2 * b2 - 16.f * c2);
    const float r2 = (b2 + sq2) / 2.f;
    const float a3 = 4.f * o;
    const float b3 = -2.f * o * (height + width);
    const float c3 = (o - 1.f) * width * height;
    const float sq3 = sqrtf(b3 * b3 - 4.f * a3 * c3);
    const float r3 = (b3 + sq3) / 2.f;
    return fminf(fminf(r1, r2), r3);
}

__global__ __launch_bounds__(256) void cp_slot_kernel(const float *__restrict__ gt_boxes, const int *__restrict__ gt_classes, CptParams p,
                                                      float *__restrict__ anno_box, int *__restrict__ ind, uint8_t *__restrict__ mask,
                                                      int *__restrict__ cat, float *__restrict__ gbc, int4 *__restrict__ draw) {
    __shared__ float box[CPT_MAX_GT * 9];
    __shared__ __attribute__((aligned(16))) int cls[CPT_MAX_GT];
    __shared__ int red[4];
    const int t = blockIdx.x, b = blockIdx.y, G = p.G, M = p.M;
    const int base = p.class_base[t], nc = p.num_classes[t];
    const float *src = gt_boxes + (size_t)b * G * 9;
    for (int i = threadIdx.x; i < G * 9; i += 256) box[i] = src[i];
    int n_before = 0, n_task = 0, n_all = 0;   // this lane's share of: rows of earlier tasks, of this task, of any task
    for (int j = threadIdx.x; j < G; j += 256) {
        const int c = gt_classes[(size_t)b * G + j];
        const bool valid = c >= 1 && c <= p.total_classes;
        cls[j] = valid ? c : CPT_INVALID;
        n_all += valid;
        n_before += valid && c <= base;
        n_task += valid && c > base && c <= base + nc;
    }
    for (int j = G + threadIdx.x; j < ((G + 3) & ~3); j += 256) cls[j] = CPT_INVALID;   // the counting loop reads four classes at a time
    n_before = block_count(n_before, red);
    n_task = block_count(n_task, red);
    n_all = block_count(n_all, red);   // (the barriers inside also publish box / cls)

    const size_t row0 = ((size_t)b * p.T + t) * M;
    int4 *dl = draw + ((size_t)b * p.T + t) * (G + 1);
    if (threadIdx.x == 0) dl[0] = make_int4(n_task, 0, 0, 0);
    const float P = 6.28318548202514648f;   // (float)(2 pi)
    for (int i = threadIdx.x; i < G; i += 256) {
        const int c = cls[i];
        if (c <= base || c > base + nc) continue;   // (CPT_INVALID is above every range)
        int less = 0;                               // rows before this one in (class, index) order: its row of gt_boxes_and_cls
        for (int j = 0; j < G; j += 4) {            // (one 16-byte LDS read per four rows: fewer dependent reads per row)
            const int4 q = *(const int4 *)(cls + j);
            less += (q.x < c || (q.x == c && j < i)) + (q.y < c || (q.y == c && j + 1 < i)) + (q.z < c || (q.z == c && j + 2 < i)) +
                    (q.w < c || (q.w == c && j + 3 < i));
        }
        const int k = less - n_before;              // slot inside the task
        const float *g = box + i * 9;
        const float x = g[0], y = g[1], z = g[2], w = g[3], l = g[4], h = g[5], vx = g[6], vy = g[7];
        const float rot = g[8] - floorf(g[8] / P + 0.5f) * P;
        float *q = gbc + ((size_t)b * M + less) * 10;
        q[0] = x; q[1] = y; q[2] = z; q[3] = w; q[4] = l; q[5] = h; q[6] = rot; q[7] = vx; q[8] = vy; q[9] = (float)c;

        const float wc = w / p.vs_x / p.osf, lc = l / p.vs_y / p.osf;
        const float ctx = (x - p.pc_x) / p.vs_x / p.osf, cty = (y - p.pc_y) / p.vs_y / p.osf;
        // clamped before the cast (a float outside int's range has no defined conversion): -1 and 2^30 are both outside every map,
        // a NaN becomes -1; values inside the map are not touched, so ct - ct_int below is the reference's
        const int cx = (int)fminf(fmaxf(ctx, -1.f), 1073741824.f), cy = (int)fminf(fmaxf(cty, -1.f), 1073741824.f);
        const bool drawn = wc > 0.f && lc > 0.f && isfinite(ctx) && isfinite(cty) && cx >= 0 && cx < p.W && cy >= 0 && cy < p.H;
        float a[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int radius = -1;
        if (drawn) {
            const float rf = gaussian_radius_f32(lc, wc, p.overlap);
            radius = max(p.min_radius, (int)fminf(rf, 1e9f));   // (clamped before the cast; 1e9 cells and more: outside the contract)
            a[0] = ctx - (float)cx; a[1] = cty - (float)cy; a[2] = z;
            a[3] = logf(w); a[4] = logf(l); a[5] = logf(h);
            a[6] = vx; a[7] = vy; a[8] = sinf(rot); a[9] = cosf(rot);
        }
        float *ab = anno_box + (row0 + k) * 10;
#pragma unroll
        for (int e = 0; e < 10; ++e) ab[e] = a[e];
        ind[row0 + k] = drawn ? cy * p.W + cx : 0;
        mask[row0 + k] = drawn ? 1 : 0;
        cat[row0 + k] = drawn ? c - base - 1 : 0;
        dl[1 + k] = make_int4(cx, cy, radius, c - base - 1);
    }
    // the slots no row of the task took, and (task 0's workgroup) the rows of gt_boxes_and_cls past the last member
    for (int k = n_task + threadIdx.x; k < M; k += 256) {
        ind[row0 + k] = 0;
        mask[row0 + k] = 0;
        cat[row0 + k] = 0;
    }
    for (int e = n_task * 10 + threadIdx.x; e < M * 10; e += 256) anno_box[row0 * 10 + e] = 0.f;
    if (t == 0)
        for (int e = n_all * 10 + threadIdx.x; e < M * 10; e += 256) gbc[(size_t)b * M * 10 + e] = 0.f;
}

__global__ __launch_bounds__(256) void cp_heat_kernel(const int4 *__restrict__ draw, CptParams p, int tiles_x, float *__restrict__ hm) {
    const int tc = blockIdx.y, b = blockIdx.z, t = tc / p.C, c = tc - t * p.C;
    const int4 *dl = draw + ((size_t)b * p.T + t) * (p.G + 1);
    const int n = c < p.num_classes[t] ? min(dl[0].x, p.G) : 0;   // a channel past the task's classes: nothing to scan, zeros are stored
    heat_tile<CPT_MAX_GT>(dl + 1, n, c, blockIdx.x, tiles_x, p.H, p.W, hm + ((size_t)b * p.T * p.C + tc) * p.H * p.W);
}

}  // namespace md

using namespace md;

// scratch of md_cp_assign_targets: draw[B][T][G + 1] int4
extern "C" int64_t md_cp_assign_targets_workspace_bytes(int64_t B, int64_t T, int64_t G) {
    return any_negative({B, T, G}) ? -1 : ws_answer((int64_t)(Sz(B) * T * (Sz(G) + 1) * 16));
}

extern "C" int md_cp_assign_targets(MD_AOT_ARGS) {
    // in : gt_boxes[B,G,9] f32, gt_classes[B,G] i32
    // out: hm[B,T,C,H,W] f32, anno_box[B,T,M,10] f32, ind[B,T,M] i32, mask[B,T,M] u8, cat[B,T,M] i32, gt_boxes_and_cls[B,M,10] f32 ;
    //      [workspace >= B T (G + 1) 16 bytes]
    Args a(MD_ARGS, 8, 9);
    const md_cp_targets_attrs *at = a.attrs<md_cp_targets_attrs>(extra);
    a.tensor(0, F32, 3); a.tensor(1, I32, 2); a.tensor(2, F32, 5); a.tensor(3, F32, 4); a.tensor(4, I32, 3); a.tensor(5, U8, 3);
    a.tensor(6, I32, 3); a.tensor(7, F32, 3); a.scratch(8);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), G = a.d(0, 1), T = a.d(2, 1), C = a.d(2, 2), H = a.d(2, 3), W = a.d(2, 4), M = a.d(3, 2);
    a.require(B >= 0 && G >= 0 && M >= 0 && H >= 1 && W >= 1 && a.d(0, 2) == 9 && a.d(1, 0) == B && a.d(1, 1) == G);
    a.require(a.d(2, 0) == B && a.d(3, 0) == B && a.d(3, 1) == T && a.d(3, 3) == 10 && a.d(7, 0) == B && a.d(7, 1) == M && a.d(7, 2) == 10);
    for (int i = 4; i <= 6; ++i) a.require(a.d(i, 0) == B && a.d(i, 1) == T && a.d(i, 2) == M);
    a.require(at->num_tasks >= 1 && at->num_tasks <= MD_CP_TARGETS_MAX_TASKS && at->num_tasks == T);
    if (int rc = a.rc()) return rc;
    CptParams p;
    int max_nc = 0, total = 0;
    for (int t = 0; t < MD_CP_TARGETS_MAX_TASKS; ++t) {
        const int nc = t < at->num_tasks ? at->num_classes[t] : 0;
        if (t < at->num_tasks) a.require(nc >= 1 && nc <= 65535);
        p.class_base[t] = total;
        p.num_classes[t] = nc;
        total += nc > 0 ? nc : 0;
        max_nc = nc > max_nc ? nc : max_nc;
    }
    a.require(C == max_nc && G <= M);
    a.require(isfinite(at->voxel_size[0]) && isfinite(at->voxel_size[1]) && at->voxel_size[0] > 0.f && at->voxel_size[1] > 0.f);
    a.require(isfinite(at->pc_range[0]) && isfinite(at->pc_range[1]) && at->out_size_factor > 0 && at->min_radius >= 0);
    a.require(at->gaussian_overlap > 0.f && at->gaussian_overlap < 1.f);   // (false for a NaN)
    if (int rc = a.rc()) return rc;
    const int64_t lim = (int64_t)1 << 30;
    if (G > CPT_MAX_GT || mul({B, G, 9}) >= lim || a.numel(2) >= lim || a.numel(3) >= lim || a.numel(7) >= lim || B > 65535 ||
        mul({T, C}) > 65535)
        return MD_ERR_SIZE;
    if (B == 0) return MD_OK;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7})) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = ws.acquire((size_t)md_cp_assign_targets_workspace_bytes(B, T, G), a, 8, s)) return rc;
    p.G = (int)G; p.M = (int)M; p.T = (int)T; p.C = (int)C; p.H = (int)H; p.W = (int)W;
    p.total_classes = total;
    p.vs_x = at->voxel_size[0]; p.vs_y = at->voxel_size[1]; p.pc_x = at->pc_range[0]; p.pc_y = at->pc_range[1];
    p.osf = (float)at->out_size_factor; p.overlap = at->gaussian_overlap; p.min_radius = at->min_radius;
    int4 *draw = (int4 *)ws.ptr;
    hipLaunchKernelGGL(cp_slot_kernel, dim3((unsigned)T, (unsigned)B), dim3(256), 0, s, (const float *)params[0], (const int *)params[1], p,
                       (float *)params[3], (int *)params[4], (uint8_t *)params[5], (int *)params[6], (float *)params[7], draw);
    const int tiles_x = (int)((W + HEAT_TILE_W - 1) / HEAT_TILE_W), tiles_y = (int)((H + HEAT_TILE_H - 1) / HEAT_TILE_H);
    hipLaunchKernelGGL(cp_heat_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)(T * C), (unsigned)B), dim3(256), 0, s, draw, p, tiles_x,
                       (float *)params[2]);
    return launched();
}
