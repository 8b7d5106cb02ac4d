// cpaug.hip -- CenterPoint (nuScenes) training input on the device (include/minddet_hip_cpaug.h; feeds md_voxelize of pillars.hip and
// md_cp_assign_targets of cptargets.hip).
//
// What it replaces: the training branch of Preprocess and the ground-truth filter of Voxelization
// (centerpoint/det3d_ms/datasets/pipelines/preprocess.py:46-157, 187-193), numpy and numba loops on the host: points_count_rbbox
// (core/bbox/box_np_ops.py:9-14), the accept step of DataBaseSamplerV2.sample_class_v2 (core/sampler/sample_ops.py:245-291) under
// sample_all (:127-185), random_flip_both / global_rotation / global_scaling_v2 / global_translate_ (core/sampler/preprocess.py:665-721,
// 812-834), filter_gt_box_outside_range (:102-116).
//   cp_count_record_kernel  one record per ground-truth box (centre, cos / sin, half extents, padded squared bounding radius) in the
//                           workspace; clears the box's count
//   cp_count_kernel         256 points per workgroup: sample by a binary search of the offsets, every point against every box of its
//                           sample behind the bounding-circle pre-test
//   cp_count_finish_kernel  keep = the min-points mask
//   cp_matrix_kernel        (sample, 16 candidate rows) per workgroup: the BEV corners of the sample's G + S boxes in LDS as float64,
//                           a wave per (row, 64 columns), one ballot = one 64-bit word of the collision matrix in the workspace
//   cp_resolve_kernel       one wave per sample: the sample's rows in LDS, lane = word of the row, a live-column mask per lane, the
//                           groups walked in order, one ballot per candidate
//   cp_points_flag_kernel   256 rows of the merged list (each sample: its candidates' points, then its scene points) per workgroup:
//                           keep flag and block count;  cp_points_scan_kernel: one workgroup, prefix of the block counts, offsets_out,
//                           the samples' transform records;  cp_points_scatter_kernel: ballot ranks, the transformed row stored once
//   cp_boxes_kernel         one wave per sample
// The point counts: integer atomics after a clear (the record kernel stores the zeros, no memset).  The alternative, per-block partial
// counts with a fixed finish, needs a [blocks][G] table written and summed -- 8 MiB at 4 x 260 000 points and G = 512 -- for hits that
// are a few per cent of the points; integer sums give the same bits in any order, so the atomics cost no determinism.
// LDS (of the 160 KiB a gfx950 workgroup has): cp_matrix_kernel 8 (512 + 256) doubles = 48 KiB of corners + 768 B of live flags;
// cp_resolve_kernel 256 x 12 words = 24 KiB of rows + 1 KiB of groups; every other kernel 16 B.  Sum of the largest: 48.75 KiB.
// Box records are read from the workspace, not LDS, as in pcaug.hip.
// Every decision and transform in float64 (fp contraction off), one rounding where an fp32 value is stored; no floating-point atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "aot.h"
#include "../../include/minddet_hip_cpaug.h"

#pragma clang fp contract(off)

#include "aug_geom.h"
#include "workgroup.h"

namespace md {

static_assert(sizeof(md_cp_count_attrs) == 4 && sizeof(md_cp_boxes_attrs) == 16, "minddet_hip_cpaug.h: attribute struct layout");

constexpr const char *F64 = "float64";
constexpr int CPA_MAX_GT = MD_CPAUG_MAX_GT, CPA_MAX_CAND = MD_CPAUG_MAX_CAND, CPA_MAX_BATCH = MD_CPAUG_MAX_BATCH;
constexpr int CPA_F = 5;         // point features
constexpr int CPA_BOX = 9;       // floats per box
constexpr int CPA_REC = 12;      // doubles per box record
constexpr int CPA_GREC = 8;      // doubles per sample record
constexpr int CPA_ROWS = 16;     // candidate rows per workgroup of cp_matrix_kernel
constexpr int CPA_MAX_WORDS = (CPA_MAX_GT + CPA_MAX_CAND + 63) / 64;
constexpr double CPA_PI = 3.141592653589793, CPA_2PI = 6.283185307179586;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ------------------------------------------------------------------------------------------------ md_cp_aug_count_points
struct CountArgs {
    const float *pts; const int *offsets; const float *boxes; const int *count;
    int *counts; uint8_t *keep; double *rec;
    int N, B, G, min_points;
};

// record: 0-2 centre, 3 cos r, 4 sin r, 5 w / 2, 6 l / 2, 7 h / 2, 8 squared bounding radius (padded), 9 the row is below gt_count
__global__ __launch_bounds__(256) void cp_count_record_kernel(CountArgs a) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)a.B * a.G) return;
    const int b = (int)(id / a.G), g = (int)(id % a.G);
    const float *q = a.boxes + id * CPA_BOX;
    double *o = a.rec + id * CPA_REC, s, c;
    sincos((double)q[8], &s, &c);
    const double hw = (double)q[3] / 2, hl = (double)q[4] / 2;
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = c; o[4] = s; o[5] = hw; o[6] = hl; o[7] = (double)q[5] / 2;
    o[8] = (hw * hw + hl * hl) * (1.0 + 1e-9);      // |l| < half extents implies d d < this: the pre-test never changes a result
    o[9] = g < clampi(a.count[b], 0, a.G) ? 1.0 : 0.0;
    o[10] = 0.0; o[11] = 0.0;
    a.counts[id] = 0;
}

__global__ __launch_bounds__(256) void cp_count_kernel(CountArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const int b = find_sample(a.offsets, a.B, i);
    if (b < 0) return;
    const float *p = a.pts + (size_t)i * CPA_F;
    const double x = p[0], y = p[1], z = p[2];
    const int cnt = clampi(a.count[b], 0, a.G);
    const double *rec = a.rec + (size_t)b * a.G * CPA_REC;
    for (int g = 0; g < cnt; ++g) {
        const double *r = rec + (size_t)g * CPA_REC;
        const double dx = x - r[0], dy = y - r[1];
        if (!(dx * dx + dy * dy < r[8])) continue;
        const double lx = dx * r[3] - dy * r[4], ly = dx * r[4] + dy * r[3], dz = z - r[2];
        if (fabs(lx) < r[5] && fabs(ly) < r[6] && fabs(dz) < r[7]) atomicAdd(a.counts + (size_t)b * a.G + g, 1);
    }
}

__global__ __launch_bounds__(256) void cp_count_finish_kernel(CountArgs a) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)a.B * a.G) return;
    const int b = (int)(id / a.G), g = (int)(id % a.G);
    const bool on = g < clampi(a.count[b], 0, a.G) && (a.min_points <= 0 || a.counts[id] >= a.min_points);
    a.keep[id] = on ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ md_cp_aug_select
struct SelectArgs {
    const float *gt; const int *gcount; const uint8_t *keep; const float *cand; const int *ccount, *group;
    uint8_t *accept; unsigned long long *bits;
    int G, S, W;
};

// bits [B][S][W]: bit j of row s = candidate s collides with column j (j < G: ground-truth row j, kept; else candidate j - G, below
// cand_count), the diagonal clear.  box_collision_test(boxes[i], qboxes[j]): the row's box is the first argument.
__global__ __launch_bounds__(256) void cp_matrix_kernel(SelectArgs a) {
    __shared__ double tab[(CPA_MAX_GT + CPA_MAX_CAND) * 8];      // x0..x3, y0..y3 per column
    __shared__ uint8_t live[CPA_MAX_GT + CPA_MAX_CAND];
    const int b = blockIdx.x, row0 = blockIdx.y * CPA_ROWS, G = a.G, S = a.S, W = a.W, C = G + S;
    const int gc = clampi(a.gcount[b], 0, G), cc = clampi(a.ccount[b], 0, S);
    const int rows = min(CPA_ROWS, S - row0);
    unsigned long long *bits = a.bits + ((size_t)b * S + row0) * W;
    if (row0 >= cc) {                             // (uniform) nothing to test: the resolve reads rows below cand_count only
        for (int k = threadIdx.x; k < rows * W; k += 256) bits[k] = 0ull;
        return;
    }
    for (int j = threadIdx.x; j < C; j += 256) {
        const bool is_gt = j < G;
        const float *q = is_gt ? a.gt + ((size_t)b * G + j) * CPA_BOX : a.cand + ((size_t)b * S + (j - G)) * CPA_BOX;
        const bool on = is_gt ? (j < gc && a.keep[(size_t)b * G + j] != 0) : (j - G < cc);
        live[j] = on ? 1 : 0;
        double s, c, x[4], y[4];
        sincos((double)q[8], &s, &c);
        rect_corners((double)q[3], (double)q[4], c, s, x, y);
        for (int m = 0; m < 4; ++m) {
            tab[j * 8 + m] = x[m] + (double)q[0];
            tab[j * 8 + 4 + m] = y[m] + (double)q[1];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int item = wave; item < rows * W; item += 4) {      // (uniform per wave)
        const int r = item / W, w = item - r * W, s = row0 + r, j = w * 64 + lane;
        bool bit = false;
        if (s < cc && j < C && live[j] && j != G + s) {
            const double *me = tab + (G + s) * 8, *other = tab + j * 8;
            bit = collide(me, me + 4, other, other + 4);
        }
        const unsigned long long bal = __ballot(bit);
        if (lane == 0) bits[item] = bal;
    }
}

// the bits j of word w with lo <= j < hi
__device__ __forceinline__ unsigned long long word_range(int w, int lo, int hi) {
    const int f = max(lo - w * 64, 0), t = min(hi - w * 64, 64);
    if (t <= f) return 0ull;
    const unsigned long long upto = t == 64 ? ~0ull : (1ull << t) - 1ull;
    return upto & ~((1ull << f) - 1ull);
}

__global__ __launch_bounds__(64) void cp_resolve_kernel(SelectArgs a) {
    __shared__ unsigned long long rows[CPA_MAX_CAND * CPA_MAX_WORDS];
    __shared__ int grp[CPA_MAX_CAND];
    const int b = blockIdx.x, lane = threadIdx.x, G = a.G, S = a.S, W = a.W;
    const int cc = clampi(a.ccount[b], 0, S);
    const int *group = a.group + (size_t)b * S;
    uint8_t *accept = a.accept + (size_t)b * S;
    bool bad = false;
    for (int i = lane; i < cc; i += 64) {
        grp[i] = group[i];
        if (i > 0 && group[i] < group[i - 1]) bad = true;
    }
    const bool skip = __ballot(bad) != 0ull;                 // a decreasing group: every candidate of the sample is rejected
    for (int s = lane; s < S; s += 64)
        if (skip || s >= cc) accept[s] = 0;
    if (skip || cc == 0) return;
    const unsigned long long *bits = a.bits + (size_t)b * S * W;
    for (int k = lane; k < cc * W; k += 64) rows[k] = bits[k];
    __syncthreads();
    // lane w keeps word w of the live columns: the ground-truth columns (the matrix holds no bit of a dropped row), the candidates
    // accepted in earlier groups, and the current group's candidates that have not been rejected
    unsigned long long alive = lane < W ? word_range(lane, 0, G) : 0ull;
    int i = 0;
    while (i < cc) {                                         // (uniform)
        int e = i + 1;
        while (e < cc && grp[e] == grp[i]) ++e;
        if (lane < W) alive |= word_range(lane, G + i, G + e);
        for (int k = i; k < e; ++k) {
            const unsigned long long row = lane < W ? rows[k * W + lane] & alive : 0ull;
            const bool hit = __ballot(row != 0ull) != 0ull;
            if (hit && lane == ((G + k) >> 6)) alive &= ~(1ull << ((G + k) & 63));      // row k and column k cleared
            if (lane == 0) accept[k] = hit ? 0 : 1;
        }
        i = e;
    }
}

// ------------------------------------------------------------------------------------------------ md_cp_aug_points
struct PtsArgs {
    const float *pts; const int *offsets; const float *cpts; const int *coffs; const float *cboxes; const uint8_t *accept;
    const double *glob;
    float *out; int *offsets_out;
    double *grec; uint8_t *flag; int *bsum;
    int N, Ns, B, S, nb;
};

__device__ __forceinline__ int pts_off(const PtsArgs &a, int b) { return clampi(a.offsets[b], 0, a.N); }
__device__ __forceinline__ int cand_off(const PtsArgs &a, int k) { return a.Ns > 0 ? clampi(a.coffs[k], 0, a.Ns) : 0; }
// first row of sample b in the merged list (b = B: its length): the candidates' points and the scene points of the samples in front
__device__ __forceinline__ int merged_start(const PtsArgs &a, int b) {
    return (cand_off(a, b * a.S) - cand_off(a, 0)) + (pts_off(a, b) - pts_off(a, 0));
}

struct MergedRow { int b, src, cand; bool keep; };      // cand: the candidate the row belongs to, -1 for a scene point
__device__ __forceinline__ MergedRow merged_row(const PtsArgs &a, int v) {
    MergedRow r = {-1, 0, -1, false};
    if (v >= a.N + a.Ns) return r;
    int lo = 0, hi = a.B + 1;                  // first sample whose start is above v
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (merged_start(a, mid) > v) hi = mid; else lo = mid + 1;
    }
    if (lo == 0 || lo == a.B + 1) return r;
    const int b = lo - 1, local = v - merged_start(a, b);
    const int c0 = cand_off(a, b * a.S), nc = cand_off(a, (b + 1) * a.S) - c0;
    r.b = b;
    if (local < nc) {
        const int ci = c0 + local;
        int l2 = 0, h2 = a.S + 1;              // first candidate boundary above ci
        while (l2 < h2) {
            const int mid = (l2 + h2) >> 1;
            if (cand_off(a, b * a.S + mid) > ci) h2 = mid; else l2 = mid + 1;
        }
        if (l2 == 0 || l2 == a.S + 1 || ci < 0 || ci >= a.Ns) return r;
        r.cand = l2 - 1;
        r.src = ci;
        r.keep = a.accept[(size_t)b * a.S + r.cand] != 0;
    } else {
        const int pi = pts_off(a, b) + (local - nc);
        if (pi < 0 || pi >= a.N || pi >= pts_off(a, b + 1)) return r;
        r.src = pi;
        r.keep = true;
    }
    return r;
}

__global__ __launch_bounds__(256) void cp_points_flag_kernel(PtsArgs a) {
    __shared__ int wcnt[4];
    const int v = blockIdx.x * 256 + threadIdx.x;
    const bool keep = merged_row(a, v).keep;
    if (v < a.N + a.Ns) a.flag[v] = keep ? 1 : 0;
    block_keep_count(keep, wcnt, a.bsum);
}

// sample record: 0 flip_a, 1 flip_b, 2 cos / 3 sin of the rotation, 4 scale, 5-7 translation
__global__ __launch_bounds__(256) void cp_points_scan_kernel(PtsArgs a) {
    __shared__ int wsum[4];
    compaction_offsets(a.bsum, a.nb, wsum);
    for (int b = threadIdx.x; b <= a.B; b += 256) {
        const int o = clampi(merged_start(a, b), 0, a.N + a.Ns), blk = o >> 8;      // blk <= nb
        int v = a.bsum[blk];
        for (int k = blk << 8; k < o; ++k) v += a.flag[k];
        a.offsets_out[b] = v;
        if (b < a.B) {
            const double *g = a.glob + (size_t)b * 7;
            double *o2 = a.grec + (size_t)b * CPA_GREC, s, c;
            sincos(g[2], &s, &c);
            o2[0] = g[0] != 0.0 ? 1.0 : 0.0; o2[1] = g[1] != 0.0 ? 1.0 : 0.0; o2[2] = c; o2[3] = s;
            o2[4] = g[3]; o2[5] = g[4]; o2[6] = g[5]; o2[7] = g[6];
        }
    }
}

__global__ __launch_bounds__(256) void cp_points_scatter_kernel(PtsArgs a) {
    __shared__ int wcnt[4];
    const int v = blockIdx.x * 256 + threadIdx.x, rows = a.N + a.Ns;
    const MergedRow r = merged_row(a, v);
    const int at = block_rank(r.keep, wcnt, a.bsum);
    const int total = a.bsum[a.nb];
    if (v < rows && v >= total) {
        float *z = a.out + (size_t)v * CPA_F;
        for (int e = 0; e < CPA_F; ++e) z[e] = 0.f;
    }
    if (!r.keep) return;
    const float *p = r.cand >= 0 ? a.cpts + (size_t)r.src * CPA_F : a.pts + (size_t)r.src * CPA_F;
    double x = p[0], y = p[1], z = p[2];
    if (r.cand >= 0) {                          // s_points[:, :3] += box3d_lidar[:3], sample_ops.py:184
        const float *q = a.cboxes + ((size_t)r.b * a.S + r.cand) * CPA_BOX;
        x += (double)q[0]; y += (double)q[1]; z += (double)q[2];
    }
    const double *g = a.grec + (size_t)r.b * CPA_GREC;
    if (g[0] != 0.0) y = -y;
    if (g[1] != 0.0) x = -x;
    const double rx = x * g[2] + y * g[3], ry = -x * g[3] + y * g[2];
    x = rx * g[4] + g[5];
    y = ry * g[4] + g[6];
    z = z * g[4] + g[7];
    if (at >= 0 && at < rows) {
        float *o = a.out + (size_t)at * CPA_F;
        o[0] = (float)x; o[1] = (float)y; o[2] = (float)z;
        for (int e = 3; e < CPA_F; ++e) o[e] = p[e];
    }
}

// ------------------------------------------------------------------------------------------------ md_cp_aug_boxes
struct BoxArgs {
    const float *gt; const int *gcls, *gcount; const uint8_t *keep; const float *cand; const int *ccls; const uint8_t *accept;
    const double *glob;
    float *out; int *out_cls, *out_count;
    int G, S;
    double xmin, ymin, xmax, ymax;
};

__global__ __launch_bounds__(64) void cp_boxes_kernel(BoxArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x, G = a.G, S = a.S, C = G + S;
    const int cnt = clampi(a.gcount[b], 0, G);
    const double *gl = a.glob + (size_t)b * 7;
    double gs, gc;
    sincos(gl[2], &gs, &gc);
    const bool flip_a = gl[0] != 0.0, flip_b = gl[1] != 0.0;
    const double scale = gl[3];
    float *out = a.out + (size_t)b * C * CPA_BOX;
    int *out_cls = a.out_cls + (size_t)b * C;
    int base = 0;
    for (int j0 = 0; j0 < C; j0 += 64) {
        const int j = j0 + lane;
        bool keep = false;
        int cls = 0;
        float o[CPA_BOX] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (j < C) {
            const bool is_gt = j < G;
            const float *q;
            bool sel;
            if (is_gt) {
                q = a.gt + ((size_t)b * G + j) * CPA_BOX;
                cls = a.gcls[(size_t)b * G + j];
                sel = j < cnt && a.keep[(size_t)b * G + j] != 0 && cls > 0;
            } else {
                q = a.cand + ((size_t)b * S + (j - G)) * CPA_BOX;
                cls = a.ccls[(size_t)b * S + (j - G)];
                sel = a.accept[(size_t)b * S + (j - G)] != 0 && cls > 0;
            }
            if (sel) {
                double x = q[0], y = q[1], z = q[2], w = q[3], l = q[4], h = q[5], vx = q[6], vy = q[7], r = q[8];
                if (flip_a) { y = -y; vy = -vy; r = -r + CPA_PI; }
                if (flip_b) { x = -x; vx = -vx; r = -r + CPA_2PI; }
                const double rx = x * gc + y * gs, ry = -x * gs + y * gc;
                const double rvx = vx * gc + vy * gs, rvy = -vx * gs + vy * gc;
                r += gl[2];
                x = rx * scale + gl[4]; y = ry * scale + gl[5]; z = z * scale + gl[6];
                w *= scale; l *= scale; h *= scale;
                vx = rvx * scale; vy = rvy * scale;
                double s, c, cx[4], cy[4];
                sincos(r, &s, &c);
                rect_corners(w, l, c, s, cx, cy);
                bool in = false;
                for (int m = 0; m < 4; ++m) {
                    const double px = cx[m] + x, py = cy[m] + y;
                    in = in || (px > a.xmin && px < a.xmax && py > a.ymin && py < a.ymax);
                }
                keep = in;
                o[0] = (float)x; o[1] = (float)y; o[2] = (float)z; o[3] = (float)w; o[4] = (float)l; o[5] = (float)h;
                o[6] = (float)vx; o[7] = (float)vy; o[8] = (float)r;
            }
        }
        const unsigned long long bal = __ballot(keep);
        if (keep) {
            const int at = base + lane_rank(bal);
            float *dst = out + (size_t)at * CPA_BOX;
            for (int e = 0; e < CPA_BOX; ++e) dst[e] = o[e];
            out_cls[at] = cls;
        }
        base += __popcll(bal);
    }
    for (int j = base + lane; j < C; j += 64) {
        for (int e = 0; e < CPA_BOX; ++e) out[(size_t)j * CPA_BOX + e] = 0.f;
        out_cls[j] = 0;
    }
    if (lane == 0) a.out_count[b] = base;
}

}  // namespace md

using namespace md;

// scratch of md_cp_aug_count_points: rec[B G][CPA_REC] f64
extern "C" int64_t md_cp_aug_count_points_workspace_bytes(int64_t B, int64_t G) {
    return any_negative({B, G}) ? -1 : ws_answer((int64_t)(Sz(B) * G * CPA_REC * 8));
}
// scratch of md_cp_aug_select: bits[B][S][ceil((G + S) / 64)] u64
extern "C" int64_t md_cp_aug_select_workspace_bytes(int64_t B, int64_t G, int64_t S) {
    return any_negative({B, G, S}) ? -1 : ws_answer((int64_t)(Sz(B) * S * ((Sz(G) + S + 63) / 64) * 8));
}
// scratch of md_cp_aug_points: grec[B][CPA_GREC] f64 at 0, bsum[ceil((N + Ns) / 256) + 1] i32, flag[N + Ns] u8
struct PtsScratch { int64_t bsum, flag, total; };
static PtsScratch cp_points_scratch(Sz N, Sz Ns, Sz B) {
    const Sz bsum = B * CPA_GREC * 8, flag = bsum + ((N + Ns + 255) / 256 + 1) * 4, total = flag + N + Ns;
    return {(int64_t)bsum, (int64_t)flag, (int64_t)total};
}
extern "C" int64_t md_cp_aug_points_workspace_bytes(int64_t N, int64_t Ns, int64_t B) {
    return any_negative({N, Ns, B}) ? -1 : ws_answer(cp_points_scratch(N, Ns, B).total);
}

extern "C" int md_cp_aug_count_points(MD_AOT_ARGS) {
    // in : points[N,5] f32, offsets[B+1] i32, gt_boxes[B,G,9] f32, gt_count[B] i32
    // out: counts[B,G] i32, keep[B,G] u8 ; [workspace]
    Args a(MD_ARGS, 6, 7);
    const md_cp_count_attrs *at = a.attrs<md_cp_count_attrs>(extra);
    a.tensor(0, F32, 2); a.tensor(1, I32, 1); a.tensor(2, F32, 3); a.tensor(3, I32, 1); a.tensor(4, I32, 2); a.tensor(5, U8, 2);
    a.scratch(6);
    if (int rc = a.rc()) return rc;
    const int64_t N = a.d(0, 0), B = a.d(1, 0) - 1, G = a.d(2, 1);
    a.require(N >= 0 && B >= 0 && G >= 0 && a.d(0, 1) == CPA_F && a.d(2, 0) == B && a.d(2, 2) == CPA_BOX && a.d(3, 0) == B);
    a.require(a.d(4, 0) == B && a.d(4, 1) == G && a.same_shape(5, 4));
    if (int rc = a.rc()) return rc;
    if (N >= ((int64_t)1 << 30) || G > CPA_MAX_GT || B > CPA_MAX_BATCH) return MD_ERR_SIZE;
    if (!a.have({1})) return MD_ERR_ARG;
    if (B > 0 && !a.have({2, 3, 4, 5})) return MD_ERR_ARG;
    if (N > 0 && !a.have({0})) return MD_ERR_ARG;
    if (aliased(params, 4, 6)) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = ws.acquire((size_t)md_cp_aug_count_points_workspace_bytes(B, G), a, 6, s)) return rc;
    if (B * G == 0) return MD_OK;
    CountArgs k;
    k.pts = (const float *)params[0]; k.offsets = (const int *)params[1]; k.boxes = (const float *)params[2];
    k.count = (const int *)params[3]; k.counts = (int *)params[4]; k.keep = (uint8_t *)params[5]; k.rec = (double *)ws.ptr;
    k.N = (int)N; k.B = (int)B; k.G = (int)G; k.min_points = at->min_points;
    const unsigned gb = (unsigned)((B * G + 255) / 256), nb = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(cp_count_record_kernel, dim3(gb), dim3(256), 0, s, k);
    if (nb > 0) hipLaunchKernelGGL(cp_count_kernel, dim3(nb), dim3(256), 0, s, k);
    hipLaunchKernelGGL(cp_count_finish_kernel, dim3(gb), dim3(256), 0, s, k);
    return launched();
}

extern "C" int md_cp_aug_select(MD_AOT_ARGS) {
    // in : gt_boxes[B,G,9] f32, gt_count[B] i32, keep[B,G] u8, cand_boxes[B,S,9] f32, cand_count[B] i32, cand_group[B,S] i32
    // out: accept[B,S] u8 ; [workspace]
    Args a(MD_ARGS, 7, 8);
    a.tensor(0, F32, 3); a.tensor(1, I32, 1); a.tensor(2, U8, 2); a.tensor(3, F32, 3); a.tensor(4, I32, 1); a.tensor(5, I32, 2);
    a.tensor(6, U8, 2); a.scratch(7);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), G = a.d(0, 1), S = a.d(3, 1);
    a.require(B >= 0 && G >= 0 && S >= 0 && a.d(0, 2) == CPA_BOX && a.d(1, 0) == B && a.d(2, 0) == B && a.d(2, 1) == G);
    a.require(a.d(3, 0) == B && a.d(3, 2) == CPA_BOX && a.d(4, 0) == B && a.d(5, 0) == B && a.d(5, 1) == S && a.same_shape(6, 5));
    if (int rc = a.rc()) return rc;
    if (G > CPA_MAX_GT || S > CPA_MAX_CAND || B > CPA_MAX_BATCH) return MD_ERR_SIZE;
    if (B > 0 && !a.have({0, 1, 2, 3, 4, 5, 6})) return MD_ERR_ARG;
    if (aliased(params, 6, 7)) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t W = (G + S + 63) / 64;
    Scratch ws;
    if (int rc = ws.acquire((size_t)md_cp_aug_select_workspace_bytes(B, G, S), a, 7, s)) return rc;
    if (B * S == 0) return MD_OK;
    SelectArgs k;
    k.gt = (const float *)params[0]; k.gcount = (const int *)params[1]; k.keep = (const uint8_t *)params[2];
    k.cand = (const float *)params[3]; k.ccount = (const int *)params[4]; k.group = (const int *)params[5];
    k.accept = (uint8_t *)params[6]; k.bits = (unsigned long long *)ws.ptr;
    k.G = (int)G; k.S = (int)S; k.W = (int)W;
    hipLaunchKernelGGL(cp_matrix_kernel, dim3((unsigned)B, (unsigned)((S + CPA_ROWS - 1) / CPA_ROWS)), dim3(256), 0, s, k);
    hipLaunchKernelGGL(cp_resolve_kernel, dim3((unsigned)B), dim3(64), 0, s, k);
    return launched();
}

extern "C" int md_cp_aug_points(MD_AOT_ARGS) {
    // in : points[N,5] f32, offsets[B+1] i32, cand_points[Ns,5] f32 | NULL, cand_offsets[B S + 1] i32 | NULL, cand_boxes[B,S,9] f32 | NULL,
    //      accept[B,S] u8 | NULL, global[B,7] f64
    // out: points_out[N+Ns,5] f32, offsets_out[B+1] i32 ; [workspace]
    Args a(MD_ARGS, 9, 10);
    a.tensor(0, F32, 2); a.tensor(1, I32, 1); a.optional(2, F32, 2); a.optional(3, I32, 1); a.optional(4, F32, 3); a.optional(5, U8, 2);
    a.tensor(6, F64, 2); a.tensor(7, F32, 2); a.tensor(8, I32, 1); a.scratch(9);
    if (int rc = a.rc()) return rc;
    const int64_t N = a.d(0, 0), B = a.d(1, 0) - 1;
    const bool cand = a.given(2);
    a.require(a.given(3) == cand && a.given(4) == cand && a.given(5) == cand);
    if (int rc = a.rc()) return rc;
    const int64_t Ns = cand ? a.d(2, 0) : 0, S = cand ? a.d(4, 1) : 0;
    a.require(N >= 0 && B >= 0 && a.d(0, 1) == CPA_F && a.d(6, 0) == B && a.d(6, 1) == 7);
    if (cand)
        a.require(Ns >= 0 && S >= 0 && a.d(2, 1) == CPA_F && a.d(3, 0) == B * S + 1 && a.d(4, 0) == B && a.d(4, 2) == CPA_BOX &&
                  a.d(5, 0) == B && a.d(5, 1) == S);
    a.require(a.d(7, 0) == N + Ns && a.d(7, 1) == CPA_F && a.same_shape(8, 1));
    if (int rc = a.rc()) return rc;
    if (N + Ns >= ((int64_t)1 << 30) || S > CPA_MAX_CAND || B > CPA_MAX_BATCH) return MD_ERR_SIZE;
    if (!a.have({1, 8})) return MD_ERR_ARG;
    if (B > 0 && !a.have({6})) return MD_ERR_ARG;
    if (N > 0 && !a.have({0})) return MD_ERR_ARG;
    if (N + Ns > 0 && !a.have({7})) return MD_ERR_ARG;
    if (aliased(params, 7, 9)) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = N + Ns, nb = (rows + 255) / 256;
    const PtsScratch w = cp_points_scratch(N, Ns, B);
    Scratch ws;
    if (int rc = ws.acquire((size_t)w.total, a, 9, s)) return rc;
    PtsArgs k;
    k.pts = (const float *)params[0]; k.offsets = (const int *)params[1];
    k.cpts = cand ? (const float *)params[2] : nullptr; k.coffs = cand ? (const int *)params[3] : nullptr;
    k.cboxes = cand ? (const float *)params[4] : nullptr; k.accept = cand ? (const uint8_t *)params[5] : nullptr;
    k.glob = (const double *)params[6]; k.out = (float *)params[7]; k.offsets_out = (int *)params[8];
    k.grec = (double *)ws.ptr; k.bsum = (int *)((char *)ws.ptr + w.bsum); k.flag = (uint8_t *)ws.ptr + w.flag;
    k.N = (int)N; k.Ns = (int)Ns; k.B = (int)B; k.S = (int)S; k.nb = (int)nb;
    if (nb > 0) hipLaunchKernelGGL(cp_points_flag_kernel, dim3((unsigned)nb), dim3(256), 0, s, k);
    hipLaunchKernelGGL(cp_points_scan_kernel, dim3(1), dim3(256), 0, s, k);
    if (nb > 0) hipLaunchKernelGGL(cp_points_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, s, k);
    return launched();
}

extern "C" int md_cp_aug_boxes(MD_AOT_ARGS) {
    // in : gt_boxes[B,G,9] f32, gt_classes[B,G] i32, gt_count[B] i32, keep[B,G] u8, cand_boxes[B,S,9] f32 | NULL,
    //      cand_classes[B,S] i32 | NULL, accept[B,S] u8 | NULL, global[B,7] f64
    // out: boxes_out[B,G+S,9] f32, classes_out[B,G+S] i32, out_count[B] i32
    Args a(MD_ARGS, 11, 11);
    const md_cp_boxes_attrs *at = a.attrs<md_cp_boxes_attrs>(extra);
    a.tensor(0, F32, 3); a.tensor(1, I32, 2); a.tensor(2, I32, 1); a.tensor(3, U8, 2); a.optional(4, F32, 3); a.optional(5, I32, 2);
    a.optional(6, U8, 2); a.tensor(7, F64, 2); a.tensor(8, F32, 3); a.tensor(9, I32, 2); a.tensor(10, I32, 1);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), G = a.d(0, 1);
    const bool cand = a.given(4);
    a.require(a.given(5) == cand && a.given(6) == cand);
    if (int rc = a.rc()) return rc;
    const int64_t S = cand ? a.d(4, 1) : 0;
    a.require(B >= 0 && G >= 0 && a.d(0, 2) == CPA_BOX && a.d(1, 0) == B && a.d(1, 1) == G && a.d(2, 0) == B && a.same_shape(3, 1));
    if (cand) a.require(S >= 0 && a.d(4, 0) == B && a.d(4, 2) == CPA_BOX && a.d(5, 0) == B && a.d(5, 1) == S && a.same_shape(6, 5));
    a.require(a.d(7, 0) == B && a.d(7, 1) == 7 && a.d(8, 0) == B && a.d(8, 1) == G + S && a.d(8, 2) == CPA_BOX);
    a.require(a.d(9, 0) == B && a.d(9, 1) == G + S && a.d(10, 0) == B);
    for (int i = 0; i < 4; ++i) a.require(isfinite(at->bv_range[i]));
    if (int rc = a.rc()) return rc;
    if (G > CPA_MAX_GT || S > CPA_MAX_CAND || B > CPA_MAX_BATCH) return MD_ERR_SIZE;
    if (B == 0) return MD_OK;
    if (!a.have({0, 1, 2, 3, 7, 8, 9, 10})) return MD_ERR_ARG;
    if (aliased(params, 8, 11)) return MD_ERR_ARG;
    BoxArgs k;
    k.gt = (const float *)params[0]; k.gcls = (const int *)params[1]; k.gcount = (const int *)params[2]; k.keep = (const uint8_t *)params[3];
    k.cand = cand ? (const float *)params[4] : nullptr; k.ccls = cand ? (const int *)params[5] : nullptr;
    k.accept = cand ? (const uint8_t *)params[6] : nullptr;
    k.glob = (const double *)params[7]; k.out = (float *)params[8]; k.out_cls = (int *)params[9]; k.out_count = (int *)params[10];
    k.G = (int)G; k.S = (int)S;
    k.xmin = at->bv_range[0]; k.ymin = at->bv_range[1]; k.xmax = at->bv_range[2]; k.ymax = at->bv_range[3];
    hipLaunchKernelGGL(cp_boxes_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, k);
    return launched();
}
