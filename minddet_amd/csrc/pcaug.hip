// pcaug.hip -- KITTI PointPillars training augmentation on the device (include/minddet_hip_pcaug.h; feeds md_voxelize of pillars.hip).
//
// What it replaces: the training branch of prep_pointcloud (minddet/models/pointpillars/src/data/preprocess.py:124-170), numba loops on
// the host: noise_per_object (src/core/preprocess.py:560-668), remove_points_in_boxes (:155-159), points_transform_ (:423-441),
// random_flip / global_rotation / global_scaling / global_translate (:671-705, 788-807), filter_gt_box_outside_range (:138-152).
//   pc_noise_kernel    one workgroup per sample, the corner table [G][4][2] in LDS, the boxes walked in order, one try per lane, every
//                      lane tests its try against the other boxes from LDS broadcast reads, a ballot picks the lowest clear try, one barrier per box
//   pc_record_kernel   one record per box (centre, cos / sin, half extents, height, squared bounding radius, transform) and one per
//                      sample (flip, cos / sin, scale, translation) in the workspace
//   pc_classify_kernel 256 points per workgroup: sample by a binary search of the offsets, owner / drop per point, the block's
//                      keep count to the workspace
//   pc_scan_kernel     one workgroup: exclusive prefix of the block counts in place, offsets_out
//   pc_scatter_kernel  ballot ranks inside the block, the transformed point stored once at its rank; zero rows behind the last
//   pc_boxes_kernel    one wave per sample
// Every decision and transform in float64 (fp contraction off), one rounding where an fp32 value is stored; no atomics, no memset.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "aot.h"
#include "../../include/minddet_hip_pcaug.h"

#pragma clang fp contract(off)

#include "aug_geom.h"      // rect_corners, covers, collide, find_sample
#include "workgroup.h"     // the compaction's block counts, scan and ranks

namespace md {

static_assert(sizeof(md_pc_boxes_attrs) == 16, "minddet_hip_pcaug.h: attribute struct layout");

constexpr const char *F64 = "float64";
constexpr int PCA_MAX_BOXES = MD_PCAUG_MAX_BOXES, PCA_MAX_TRIES = MD_PCAUG_MAX_TRIES, PCA_MAX_BATCH = MD_PCAUG_MAX_BATCH;
constexpr int PCA_REC = 16;      // doubles per box record
constexpr int PCA_GREC = 8;      // doubles per sample record
constexpr double PCA_PI = 3.141592653589793, PCA_2PI = 6.283185307179586;

struct NoiseArgs {
    const float *boxes; const int *count; const uint8_t *valid; const double *loc, *rot, *grot;
    int *selected; double *tf; float *out;
    int G, T;
};

__global__ __launch_bounds__(PCA_MAX_TRIES) void pc_noise_kernel(NoiseArgs a) {
    __shared__ double tab[PCA_MAX_BOXES * 8];      // x0..x3, y0..y3 per box
    // One barrier per box.  The tries' corners and the waves' ballots are kept in two buffers used in turn: after the barrier every lane
    // knows the winning try, its lane alone writes row i of the table, and the next box reads row i from the winner's slot of the
    // previous buffer instead; the table row is in place one barrier later, before that buffer is written again.
    __shared__ double cand[2][PCA_MAX_TRIES * 8];
    __shared__ unsigned long long bal[2][PCA_MAX_TRIES / 64];
    int par = 0, prev = -1, prev_win = 0;          // (uniform) buffer of this box; the box whose new row is still in cand[par ^ 1][prev_win]
    const int b = blockIdx.x, G = a.G, T = a.T, j = threadIdx.x, lane = j & 63, wave = j >> 6;
    const int cnt = min(max(a.count[b], 0), G);
    const float *boxes = a.boxes + (size_t)b * G * 7;
    int *selected = a.selected + (size_t)b * G;
    double *tf = a.tf + (size_t)b * G * 4;
    float *out = a.out + (size_t)b * G * 7;
    for (int g = cnt + j; g < G; g += PCA_MAX_TRIES) {
        selected[g] = -1;
        for (int e = 0; e < 4; ++e) tf[g * 4 + e] = 0.0;
        for (int e = 0; e < 7; ++e) out[g * 7 + e] = 0.f;
    }
    for (int g = j; g < cnt; g += PCA_MAX_TRIES) {
        const float *q = boxes + g * 7;
        double s, c, x[4], y[4];
        sincos((double)q[6], &s, &c);
        rect_corners((double)q[3], (double)q[4], c, s, x, y);
        for (int m = 0; m < 4; ++m) {
            tab[g * 8 + m] = x[m] + (double)q[0];
            tab[g * 8 + 4 + m] = y[m] + (double)q[1];
        }
    }
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
        const float *q = boxes + i * 7;
        if (!a.valid[(size_t)b * G + i]) {          // (uniform: no barrier is skipped by part of the workgroup)
            if (j == 0) {
                selected[i] = -1;
                for (int e = 0; e < 4; ++e) tf[i * 4 + e] = 0.0;
                for (int e = 0; e < 7; ++e) out[i * 7 + e] = q[e];
            }
            continue;
        }
        const double bx = q[0], by = q[1], bw = q[3], bl = q[4], br = q[6];
        double cx[4], cy[4], lx = 0, ly = 0, lz = 0, rn = 0;
        bool clear = j < T;
        if (j < T) {
            const size_t t = ((size_t)b * G + i) * T + j;
            lx = a.loc[t * 3]; ly = a.loc[t * 3 + 1]; lz = a.loc[t * 3 + 2];
            rn = a.rot[t];
            double px = bx, py = by, r = br;
            if (a.grot) {
                // noise_per_box_v2_, :389-396, 417-418: the centre turned about the origin by the try's angle g, where the reference
                // takes radius sin / cos of atan2(x, y) + g.  The displacement is formed directly, x (cos g - 1) + y sin g and
                // y (cos g - 1) - x sin g with cos g - 1 = -2 sin^2(g / 2): the same quantity without the cancellation of two
                // radius-sized terms, so it is good to a few ulp of its own size
                const double g = a.grot[t], sg = sin(g), sh = sin(0.5 * g), cm1 = -2.0 * sh * sh;
                const double dx = bx * cm1 + by * sg, dy = by * cm1 - bx * sg;
                px = bx + dx;
                py = by + dy;
                r = br + g;
                lx += dx;
                ly += dy;
                rn += g;
            }
            double s, c, s2, c2, x[4], y[4];
            sincos(r, &s, &c);
            rect_corners(bw, bl, c, s, x, y);
            sincos(a.rot[t], &s2, &c2);
            for (int m = 0; m < 4; ++m) {
                cx[m] = (x[m] * c2 + y[m] * s2) + (px + a.loc[t * 3]);
                cy[m] = (-x[m] * s2 + y[m] * c2) + (py + a.loc[t * 3 + 1]);
            }
            for (int m = 0; m < 4; ++m) {
                cand[par][j * 8 + m] = cx[m];
                cand[par][j * 8 + 4 + m] = cy[m];
            }
            for (int k = 0; k < cnt && clear; ++k) {
                if (k == i) continue;
                const double *row = k == prev ? cand[par ^ 1] + prev_win * 8 : tab + k * 8;
                if (collide(cx, cy, row, row + 4)) clear = false;
            }
        }
        const unsigned long long mine = __ballot(clear);
        if (lane == 0) bal[par][wave] = mine;
        __syncthreads();
        int win = -1;
        for (int w = PCA_MAX_TRIES / 64 - 1; w >= 0; --w)
            if (bal[par][w]) win = w * 64 + __ffsll((long long)bal[par][w]) - 1;
        if (j == win) {
            for (int m = 0; m < 4; ++m) {
                tab[i * 8 + m] = cx[m];
                tab[i * 8 + 4 + m] = cy[m];
            }
            selected[i] = j;
            tf[i * 4] = lx; tf[i * 4 + 1] = ly; tf[i * 4 + 2] = lz; tf[i * 4 + 3] = rn;
            out[i * 7] = (float)((double)q[0] + lx);
            out[i * 7 + 1] = (float)((double)q[1] + ly);
            out[i * 7 + 2] = (float)((double)q[2] + lz);
            out[i * 7 + 3] = q[3]; out[i * 7 + 4] = q[4]; out[i * 7 + 5] = q[5];
            out[i * 7 + 6] = (float)((double)q[6] + rn);
        } else if (win < 0 && j == 0) {
            selected[i] = -1;
            for (int e = 0; e < 4; ++e) tf[i * 4 + e] = 0.0;
            for (int e = 0; e < 7; ++e) out[i * 7 + e] = q[e];
        }
        prev = win >= 0 ? i : -1;
        prev_win = win;
        par ^= 1;
    }
}

struct PointArgs {
    const float4 *pts; const int *offsets;
    const float *obj; const int *count; const uint8_t *valid; const double *tf;
    const float *rem; const int *rem_count, *rem_from;
    const double *glob;
    float4 *out; int *offsets_out, *owner;
    double *rec, *grec; int *bsum;
    int N, B, G, R, nb;
};

// record: 0-2 centre, 3 cos r, 4 sin r, 5 w / 2, 6 l / 2, 7 h, 8 squared bounding radius (padded), 9-11 loc, 12 cos / 13 sin of the
// transform's angle, 14 transform is not the identity, 15 the box takes part
__global__ __launch_bounds__(256) void pc_record_kernel(PointArgs a) {
    const int S = a.G + a.R;
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)a.B * (S + 1)) return;
    const int b = (int)(id / (S + 1)), slot = (int)(id % (S + 1));
    if (slot == S) {
        const double *g = a.glob + (size_t)b * 6;
        double *o = a.grec + (size_t)b * PCA_GREC, s, c;
        sincos(g[1], &s, &c);
        o[0] = g[0] != 0.0 ? 1.0 : 0.0; o[1] = c; o[2] = s; o[3] = g[2]; o[4] = g[3]; o[5] = g[4]; o[6] = g[5]; o[7] = 0.0;
        return;
    }
    const bool is_obj = slot < a.G;
    const float *q = is_obj ? a.obj + ((size_t)b * a.G + slot) * 7 : a.rem + ((size_t)b * a.R + (slot - a.G)) * 7;
    double *o = a.rec + ((size_t)b * S + slot) * PCA_REC, s, c;
    sincos((double)q[6], &s, &c);
    const double hw = (double)q[3] / 2, hl = (double)q[4] / 2;
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = c; o[4] = s; o[5] = hw; o[6] = hl; o[7] = q[5];
    o[8] = (hw * hw + hl * hl) * (1.0 + 1e-9);      // |l| < half extents implies d d < this: the pre-test never changes a result
    bool on;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    if (is_obj) {
        on = slot < min(max(a.count[b], 0), a.G) && a.valid[(size_t)b * a.G + slot] != 0;
        for (int e = 0; e < 4; ++e) t[e] = a.tf[((size_t)b * a.G + slot) * 4 + e];
    } else {
        on = slot - a.G < min(max(a.rem_count[b], 0), a.R);
    }
    sincos(t[3], &s, &c);
    o[9] = t[0]; o[10] = t[1]; o[11] = t[2]; o[12] = c; o[13] = s;
    o[14] = (t[0] != 0.0 || t[1] != 0.0 || t[2] != 0.0 || t[3] != 0.0) ? 1.0 : 0.0;
    o[15] = on ? 1.0 : 0.0;
}

__device__ __forceinline__ bool inside_box(const double *r, double x, double y, double z) {
    const double dx = x - r[0], dy = y - r[1], dz = z - r[2];
    if (!(dx * dx + dy * dy < r[8])) return false;
    const double lx = dx * r[3] - dy * r[4], ly = dx * r[4] + dy * r[3];
    return fabs(lx) < r[5] && fabs(ly) < r[6] && dz > 0 && dz < r[7];
}

__global__ __launch_bounds__(256) void pc_classify_kernel(PointArgs a) {
    __shared__ int wcnt[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int b = find_sample(a.offsets, a.B, i);
    int own = -2;
    if (i < a.N && b >= 0) {
        const float4 p = a.pts[i];
        const double x = p.x, y = p.y, z = p.z;
        const int S = a.G + a.R;
        const double *rec = a.rec + (size_t)b * S * PCA_REC;
        bool drop = false;
        if (a.R > 0 && i - a.offsets[b] >= a.rem_from[b]) {
            const int rc = min(max(a.rem_count[b], 0), a.R);
            for (int r = 0; r < rc && !drop; ++r) drop = inside_box(rec + (size_t)(a.G + r) * PCA_REC, x, y, z);
        }
        if (!drop) {
            own = -1;
            const int cnt = min(max(a.count[b], 0), a.G);
            for (int g = 0; g < cnt; ++g) {
                const double *r = rec + (size_t)g * PCA_REC;
                if (r[15] != 0.0 && inside_box(r, x, y, z)) { own = g; break; }
            }
        }
    }
    if (i < a.N) a.owner[i] = own;
    block_keep_count(own != -2, wcnt, a.bsum);
}

__global__ __launch_bounds__(256) void pc_scan_kernel(PointArgs a) {
    __shared__ int wsum[4];
    compaction_offsets(a.bsum, a.nb, wsum);
    for (int b = threadIdx.x; b <= a.B; b += 256) {
        const int o = min(max(a.offsets[b], 0), a.N), blk = o >> 8;      // blk <= nb
        int v = a.bsum[blk];
        for (int k = blk << 8; k < o; ++k) v += a.owner[k] != -2;
        a.offsets_out[b] = v;
    }
}

__global__ __launch_bounds__(256) void pc_scatter_kernel(PointArgs a) {
    __shared__ int wcnt[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int b = find_sample(a.offsets, a.B, i);
    const int own = i < a.N ? a.owner[i] : -2;
    const bool keep = own != -2;
    const int at = block_rank(keep, wcnt, a.bsum);
    const int total = a.bsum[a.nb];
    if (i < a.N && i >= total) a.out[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!keep || b < 0) return;
    const float4 p = a.pts[i];
    double x = p.x, y = p.y, z = p.z;
    if (own >= 0) {
        const double *r = a.rec + ((size_t)b * (a.G + a.R) + own) * PCA_REC;
        if (r[14] != 0.0) {          // points_transform_, :437-440
            const double dx = x - r[0], dy = y - r[1], dz = z - r[2];
            x = ((dx * r[12] + dy * r[13]) + r[0]) + r[9];
            y = ((-dx * r[13] + dy * r[12]) + r[1]) + r[10];
            z = (dz + r[2]) + r[11];
        }
    }
    const double *g = a.grec + (size_t)b * PCA_GREC;
    if (g[0] != 0.0) y = -y;
    const double rx = x * g[1] + y * g[2], ry = -x * g[2] + y * g[1];
    x = rx * g[3] + g[4];
    y = ry * g[3] + g[5];
    z = z * g[3] + g[6];
    if (at >= 0 && at < a.N) a.out[at] = make_float4((float)x, (float)y, (float)z, p.w);
}

struct BoxArgs {
    const float *boxes; const int *count; const uint8_t *valid; const int *classes; const double *glob;
    float *out; int *out_classes, *out_count;
    int G;
    double xmin, ymin, xmax, ymax;
};

__global__ __launch_bounds__(64) void pc_boxes_kernel(BoxArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x, G = a.G;
    const int cnt = min(max(a.count[b], 0), G);
    const double *gl = a.glob + (size_t)b * 6;
    double gs, gc;
    sincos(gl[1], &gs, &gc);
    const bool flip = gl[0] != 0.0;
    int base = 0;
    for (int g0 = 0; g0 < cnt; g0 += 64) {
        const int g = g0 + lane;
        bool keep = false;
        float o[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (g < cnt) {
            const float *q = a.boxes + ((size_t)b * G + g) * 7;
            double x = q[0], y = q[1], z = q[2], w = q[3], l = q[4], h = q[5], r = q[6];
            if (flip) { y = -y; r = -r + PCA_PI; }
            const double rx = x * gc + y * gs, ry = -x * gs + y * gc;
            r += gl[1];
            x = rx * gl[2] + gl[3]; y = ry * gl[2] + gl[4]; z = z * gl[2] + gl[5];
            w *= gl[2]; l *= gl[2]; h *= gl[2];
            double s, c, cx[4], cy[4];
            sincos(r, &s, &c);
            rect_corners(w, l, c, s, cx, cy);
            bool in = false;
            for (int m = 0; m < 4; ++m) {
                const double px = cx[m] + x, py = cy[m] + y;
                in = in || (px > a.xmin && px < a.xmax && py > a.ymin && py < a.ymax);
            }
            keep = in && a.valid[(size_t)b * G + g] != 0;
            r = r - floor(r / PCA_2PI + 0.5) * PCA_2PI;
            o[0] = (float)x; o[1] = (float)y; o[2] = (float)z; o[3] = (float)w; o[4] = (float)l; o[5] = (float)h; o[6] = (float)r;
        }
        const unsigned long long bal = __ballot(keep);
        if (keep) {
            const int at = base + lane_rank(bal);
            float *dst = a.out + ((size_t)b * G + at) * 7;
            for (int e = 0; e < 7; ++e) dst[e] = o[e];
            a.out_classes[(size_t)b * G + at] = a.classes[(size_t)b * G + g];
        }
        base += __popcll(bal);
    }
    for (int g = base + lane; g < G; g += 64) {
        for (int e = 0; e < 7; ++e) a.out[((size_t)b * G + g) * 7 + e] = 0.f;
        a.out_classes[(size_t)b * G + g] = 0;
    }
    if (lane == 0) a.out_count[b] = base;
}

}  // namespace md

using namespace md;

extern "C" int md_pc_noise_per_object(MD_AOT_ARGS) {
    // in : gt_boxes[B,G,7] f32, gt_count[B] i32, valid[B,G] u8, loc_noises[B,G,T,3] f64, rot_noises[B,G,T] f64, grot_noises[B,G,T] f64 | NULL
    // out: selected[B,G] i32, obj_transform[B,G,4] f64, boxes_out[B,G,7] f32
    Args a(MD_ARGS, 9, 9);
    a.tensor(0, F32, 3); a.tensor(1, I32, 1); a.tensor(2, U8, 2); a.tensor(3, F64, 4); a.tensor(4, F64, 3); a.optional(5, F64, 3);
    a.tensor(6, I32, 2); a.tensor(7, F64, 3); a.tensor(8, F32, 3);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), G = a.d(0, 1), T = a.d(3, 2);
    a.require(B >= 0 && G >= 0 && T >= 1 && a.d(0, 2) == 7 && a.d(1, 0) == B && a.d(2, 0) == B && a.d(2, 1) == G);
    a.require(a.d(3, 0) == B && a.d(3, 1) == G && a.d(3, 3) == 3 && a.d(4, 0) == B && a.d(4, 1) == G && a.d(4, 2) == T);
    if (a.given(5)) a.require(a.same_shape(5, 4));
    a.require(a.d(6, 0) == B && a.d(6, 1) == G && a.d(7, 0) == B && a.d(7, 1) == G && a.d(7, 2) == 4 && a.same_shape(8, 0));
    if (int rc = a.rc()) return rc;
    if (G > PCA_MAX_BOXES || T > PCA_MAX_TRIES || B > PCA_MAX_BATCH) return MD_ERR_SIZE;
    if (B == 0) return MD_OK;
    if (!a.have({0, 1, 2, 3, 4, 6, 7, 8})) return MD_ERR_ARG;
    for (int o = 6; o <= 8; ++o)                        // box rows and draws are read after earlier boxes' outputs are stored
        for (int in = 0; in <= 5; ++in)
            if (params[o] == params[in]) return MD_ERR_ARG;
    NoiseArgs k;
    k.boxes = (const float *)params[0]; k.count = (const int *)params[1]; k.valid = (const uint8_t *)params[2];
    k.loc = (const double *)params[3]; k.rot = (const double *)params[4]; k.grot = (const double *)params[5];
    k.selected = (int *)params[6]; k.tf = (double *)params[7]; k.out = (float *)params[8];
    k.G = (int)G; k.T = (int)T;
    hipLaunchKernelGGL(pc_noise_kernel, dim3((unsigned)B), dim3(PCA_MAX_TRIES), 0, (hipStream_t)stream, k);
    return launched();
}

// scratch of md_pc_augment_points: rec[B (G + R)][PCA_REC] f64 at 0, grec[B][PCA_GREC] f64, bsum[ceil(N / 256) + 1] i32
struct PointScratch { int64_t grec, bsum, total; };
static PointScratch pc_points_scratch(Sz N, Sz B, Sz G, Sz R) {
    const Sz grec = B * (G + R) * PCA_REC * 8, bsum = grec + B * PCA_GREC * 8, total = bsum + ((N + 255) / 256 + 1) * 4;
    return {(int64_t)grec, (int64_t)bsum, (int64_t)total};
}
extern "C" int64_t md_pc_augment_points_workspace_bytes(int64_t N, int64_t B, int64_t G, int64_t R) {
    return any_negative({N, B, G, R}) ? -1 : ws_answer(pc_points_scratch(N, B, G, R).total);
}

extern "C" int md_pc_augment_points(MD_AOT_ARGS) {
    // in : points[N,4] f32, offsets[B+1] i32, obj_boxes[B,G,7] f32, gt_count[B] i32, valid[B,G] u8, obj_transform[B,G,4] f64,
    //      remove_boxes[B,R,7] f32 | NULL, remove_count[B] i32 | NULL, remove_from[B] i32 | NULL, global[B,6] f64
    // out: points_out[N,4] f32, offsets_out[B+1] i32, owner[N] i32 ; [workspace]
    Args a(MD_ARGS, 13, 14);
    a.tensor(0, F32, 2); a.tensor(1, I32, 1); a.tensor(2, F32, 3); a.tensor(3, I32, 1); a.tensor(4, U8, 2); a.tensor(5, F64, 3);
    a.optional(6, F32, 3); a.optional(7, I32, 1); a.optional(8, I32, 1); a.tensor(9, F64, 2);
    a.tensor(10, F32, 2); a.tensor(11, I32, 1); a.tensor(12, I32, 1); a.scratch(13);
    if (int rc = a.rc()) return rc;
    const int64_t N = a.d(0, 0), B = a.d(1, 0) - 1, G = a.d(2, 1);
    const bool rem = a.given(6);
    a.require(a.given(7) == rem && a.given(8) == rem);
    const int64_t R = rem ? a.d(6, 1) : 0;
    a.require(N >= 0 && B >= 0 && G >= 0 && a.d(0, 1) == 4 && a.d(2, 0) == B && a.d(2, 2) == 7 && a.d(3, 0) == B);
    a.require(a.d(4, 0) == B && a.d(4, 1) == G && a.d(5, 0) == B && a.d(5, 1) == G && a.d(5, 2) == 4);
    if (rem) a.require(R >= 0 && a.d(6, 0) == B && a.d(6, 2) == 7 && a.d(7, 0) == B && a.d(8, 0) == B);
    a.require(a.d(9, 0) == B && a.d(9, 1) == 6 && a.same_shape(10, 0) && a.same_shape(11, 1) && a.d(12, 0) == N);
    if (int rc = a.rc()) return rc;
    if (N >= ((int64_t)1 << 30) || G > PCA_MAX_BOXES || R > PCA_MAX_BOXES || B > PCA_MAX_BATCH) return MD_ERR_SIZE;
    if (!a.have({1, 11})) return MD_ERR_ARG;
    if (B > 0 && !a.have({2, 3, 4, 5, 9})) return MD_ERR_ARG;
    if (N > 0 && !a.have({0, 10, 12})) return MD_ERR_ARG;
    for (int o = 10; o <= 12; ++o)                      // the scatter reads points, offsets and owner while the outputs are stored
        for (int in = 0; in <= 9; ++in)
            if (params[o] && params[o] == params[in]) return MD_ERR_ARG;
    if (params[10] == params[12] || params[11] == params[12] || params[10] == params[11]) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (N + 255) / 256;
    const PointScratch w = pc_points_scratch(N, B, G, R);
    Scratch ws;
    if (int rc = ws.acquire((size_t)w.total, a, 13, s)) return rc;
    PointArgs k;
    k.pts = (const float4 *)params[0]; k.offsets = (const int *)params[1]; k.obj = (const float *)params[2];
    k.count = (const int *)params[3]; k.valid = (const uint8_t *)params[4]; k.tf = (const double *)params[5];
    k.rem = rem ? (const float *)params[6] : nullptr; k.rem_count = rem ? (const int *)params[7] : nullptr;
    k.rem_from = rem ? (const int *)params[8] : nullptr;
    k.glob = (const double *)params[9];
    k.out = (float4 *)params[10]; k.offsets_out = (int *)params[11]; k.owner = (int *)params[12];
    k.rec = (double *)ws.ptr; k.grec = (double *)((char *)ws.ptr + w.grec); k.bsum = (int *)((char *)ws.ptr + w.bsum);
    k.N = (int)N; k.B = (int)B; k.G = (int)G; k.R = (int)R; k.nb = (int)nb;
    if (B > 0) hipLaunchKernelGGL(pc_record_kernel, dim3((unsigned)((B * (G + R + 1) + 255) / 256)), dim3(256), 0, s, k);
    if (nb > 0) hipLaunchKernelGGL(pc_classify_kernel, dim3((unsigned)nb), dim3(256), 0, s, k);
    hipLaunchKernelGGL(pc_scan_kernel, dim3(1), dim3(256), 0, s, k);
    if (nb > 0) hipLaunchKernelGGL(pc_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, s, k);
    return launched();
}

extern "C" int md_pc_augment_boxes(MD_AOT_ARGS) {
    // in : boxes[B,G,7] f32, gt_count[B] i32, valid[B,G] u8, classes[B,G] i32, global[B,6] f64
    // out: gt_boxes[B,G,7] f32, gt_classes[B,G] i32, out_count[B] i32
    Args a(MD_ARGS, 8, 8);
    const md_pc_boxes_attrs *at = a.attrs<md_pc_boxes_attrs>(extra);
    a.tensor(0, F32, 3); a.tensor(1, I32, 1); a.tensor(2, U8, 2); a.tensor(3, I32, 2); a.tensor(4, F64, 2);
    a.tensor(5, F32, 3); a.tensor(6, I32, 2); a.tensor(7, I32, 1);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), G = a.d(0, 1);
    a.require(B >= 0 && G >= 0 && a.d(0, 2) == 7 && a.d(1, 0) == B && a.d(2, 0) == B && a.d(2, 1) == G && a.same_shape(3, 2));
    a.require(a.d(4, 0) == B && a.d(4, 1) == 6 && a.same_shape(5, 0) && a.same_shape(6, 2) && a.d(7, 0) == B);
    for (int i = 0; i < 4; ++i) a.require(isfinite(at->bv_range[i]));
    if (int rc = a.rc()) return rc;
    if (G > PCA_MAX_BOXES || B > PCA_MAX_BATCH) return MD_ERR_SIZE;
    if (B == 0) return MD_OK;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7})) return MD_ERR_ARG;
    for (int o = 5; o <= 7; ++o)                        // the compaction stores rows other lanes still read
        for (int in = 0; in <= 4; ++in)
            if (params[o] == params[in]) return MD_ERR_ARG;
    BoxArgs k;
    k.boxes = (const float *)params[0]; k.count = (const int *)params[1]; k.valid = (const uint8_t *)params[2];
    k.classes = (const int *)params[3]; k.glob = (const double *)params[4];
    k.out = (float *)params[5]; k.out_classes = (int *)params[6]; k.out_count = (int *)params[7];
    k.G = (int)G;
    k.xmin = at->bv_range[0]; k.ymin = at->bv_range[1]; k.xmax = at->bv_range[2]; k.ymax = at->bv_range[3];
    hipLaunchKernelGGL(pc_boxes_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, k);
    return launched();
}
