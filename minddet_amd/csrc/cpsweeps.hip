// cpsweeps.hip -- CenterPoint (nuScenes) multi-sweep input on the device (include/minddet_hip_cpsweeps.h; feeds md_voxelize of
// pillars.hip and md_cp_aug_* of cpaug.hip).
//
// What it replaces: read_sweep (remove_close, the 4x4 into the key frame, the time column) per past sweep and the concatenation of
// LoadPointCloudFromFile.__call__, nuScenes branch (centerpoint/det3d_ms/datasets/pipelines/loading.py:56-80, 133-159), numpy on the
// host; the reference's deployment demo does it with cupy (tools_ms/multi_sweep_inference_ros.py:194-270).
//
// One stable compaction over a virtual row space: the segments of all samples end to end, every segment padded to whole workgroups of
// 256 rows, so a workgroup lies in ONE segment and the segment's matrix, time and flags are uniform in it.  The segment lengths are
// device operands: the grid is sized from the host-known bound ceil(N / 256) + B S (the segments hold at most N rows together, each
// wastes less than one workgroup), every workgroup finds its (segment, first row) by a workgroup scan of the B S lengths (seg_walk;
// B S is 40 in the nuScenes config, the scan is a few hundred bytes of L2 per workgroup), workgroups past the end keep nothing.
//   cps_count_kernel    the keep decision of 256 rows, the workgroup's count (block_keep_count)
//   cps_scan_kernel     one workgroup: the prefix of the counts (compaction_offsets); offsets_out[b] = the prefix at the first
//                       workgroup of sample b's first segment; status
//   cps_scatter_kernel  the keep decision again (8 bytes of a row: cheaper than a flag array written and read), ballot ranks
//                       (block_rank), the row transformed and stored once; the zero rows from the total to M, grid-stride
// Validity (a range outside [0, N], more than N rows together) is evaluated by every workgroup from the same operands (seg_validate),
// so the three launches agree; an invalid sample's segments have length 0.  A row index is compared with N again before it is loaded.
// LDS: 1 KiB of per-sample flags + 64 B.  Float64 without contraction: the sum is the contract's sum, term by term.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "aot.h"
#include "../../include/minddet_hip_cpsweeps.h"

#pragma clang fp contract(off)

#include "workgroup.h"

namespace md {

static_assert(sizeof(md_cp_sweeps_attrs) == 8, "minddet_hip_cpsweeps.h: attribute struct layout");

constexpr int CPS_MAX_SWEEPS = MD_CPSWEEPS_MAX_SWEEPS, CPS_MAX_BATCH = MD_CPSWEEPS_MAX_BATCH;
constexpr int CPS_F = 5;          // output point features

struct SweepArgs {
    const float *pts; const int *range; const double *tf, *lag; const int *flags;
    float *out; int *offsets_out, *status;
    int *bsum;
    int N, Fin, M, B, S, nb;
    float radius;
};
struct SegLds {
    int bad[CPS_MAX_BATCH];       // a range of the sample leaves [0, N]
    long long part[4];
    int wsum[4];
    int found[2];                 // the workgroup's segment, its first row / 256
};

// rows of segment k; bad: its begin or end lies outside [0, N]
__device__ __forceinline__ int seg_len(const SweepArgs &a, int k, bool &bad, int &begin) {
    const int b0 = a.range[2 * k], e0 = a.range[2 * k + 1];
    bad = b0 < 0 || b0 > a.N || e0 < 0 || e0 > a.N;
    begin = b0;
    return bad ? 0 : max(e0 - b0, 0);
}

// the per-sample flags in l.bad; returns whether the in-range segments hold more than N rows.  Every lane calls; two barriers
__device__ __forceinline__ bool seg_validate(const SweepArgs &a, SegLds &l) {
    const int BS = a.B * a.S;
    for (int b = threadIdx.x; b < a.B; b += 256) l.bad[b] = 0;
    if (threadIdx.x == 0) { l.found[0] = -1; l.found[1] = 0; }
    __syncthreads();
    long long rows = 0;
    for (int k = threadIdx.x; k < BS; k += 256) {
        bool bad; int begin;
        const int len = seg_len(a, k, bad, begin);
        if (bad) atomicOr(&l.bad[k / a.S], 1);
        rows += len;
    }
    rows = wave_sum_all(rows);
    if ((threadIdx.x & 63) == 0) l.part[threadIdx.x >> 6] = rows;
    __syncthreads();
    return l.part[0] + l.part[1] + l.part[2] + l.part[3] > (long long)a.N;
}

// f(k, first workgroup of segment k, its workgroups) for the segments in order, 256 at a time, until more than `stop` workgroups are
// counted (uniform).  Every lane calls; block_exclusive_scan's barriers
template <typename F> __device__ __forceinline__ void seg_walk(const SweepArgs &a, SegLds &l, bool over, int stop, F f) {
    const int BS = a.B * a.S;
    int carry = 0;
    for (int base = 0; base < BS; base += 256) {
        const int k = base + threadIdx.x;
        int nblk = 0;
        if (k < BS && !over && !l.bad[k / a.S]) {
            bool bad; int begin;
            nblk = (seg_len(a, k, bad, begin) + 255) >> 8;
        }
        int all;
        const int ex = block_exclusive_scan<4>(nblk, l.wsum, all);
        if (k < BS) f(k, carry + ex, nblk);
        carry += all;
        if (carry > stop) break;
    }
}

struct SegRow { int k, src; bool keep; };      // k: the segment (uniform, -1: the workgroup lies past the end); src: the row of points
__device__ __forceinline__ SegRow seg_row(const SweepArgs &a, SegLds &l) {
    const bool over = seg_validate(a, l);
    const int blk = blockIdx.x;
    seg_walk(a, l, over, blk, [&](int k, int first, int nblk) {
        if (blk >= first && blk < first + nblk) { l.found[0] = k; l.found[1] = blk - first; }
    });
    __syncthreads();
    SegRow r = {__builtin_amdgcn_readfirstlane(l.found[0]), 0, false};
    if (r.k < 0) return r;
    bool bad; int begin;
    const int len = seg_len(a, r.k, bad, begin), local = l.found[1] * 256 + (int)threadIdx.x;
    r.src = begin + local;
    if (bad || local >= len || r.src < 0 || r.src >= a.N) return r;
    const float *p = a.pts + (size_t)r.src * a.Fin;
    r.keep = !((a.flags[r.k] & 1) && fabsf(p[0]) < a.radius && fabsf(p[1]) < a.radius);
    return r;
}

__global__ __launch_bounds__(256) void cps_count_kernel(SweepArgs a) {
    __shared__ SegLds l;
    __shared__ int wcnt[4];
    block_keep_count(seg_row(a, l).keep, wcnt, a.bsum);
}

__global__ __launch_bounds__(256) void cps_scan_kernel(SweepArgs a) {
    __shared__ SegLds l;
    compaction_offsets(a.bsum, a.nb, l.wsum);
    const bool over = seg_validate(a, l);
    seg_walk(a, l, over, 0x7fffffff, [&](int k, int first, int nblk) {
        if (k % a.S == 0) a.offsets_out[k / a.S] = a.bsum[min(first, a.nb)];
    });
    for (int b = threadIdx.x; b <= a.B; b += 256) {
        if (b == a.B || a.S == 0) a.offsets_out[b] = a.bsum[a.nb];      // (no segments: nothing is kept, the total is 0)
        if (b < a.B) a.status[b] = (l.bad[b] ? 1 : 0) | (over ? 2 : 0);
    }
}

__global__ __launch_bounds__(256) void cps_scatter_kernel(SweepArgs a) {
    __shared__ SegLds l;
    __shared__ int wcnt[4];
    const SegRow r = seg_row(a, l);
    const int at = block_rank(r.keep, wcnt, a.bsum);
    const int total = a.bsum[a.nb];
    for (int64_t v = (int64_t)total + (int64_t)blockIdx.x * 256 + threadIdx.x; v < a.M; v += (int64_t)gridDim.x * 256) {
        float *z = a.out + (size_t)v * CPS_F;
        for (int e = 0; e < CPS_F; ++e) z[e] = 0.f;
    }
    if (!r.keep || at < 0 || at >= a.M) return;
    const float *p = a.pts + (size_t)r.src * a.Fin;
    const float x = p[0], y = p[1], z = p[2];
    float ox = x, oy = y, oz = z;
    if (a.flags[r.k] & 2) {                                  // (uniform: the segment's matrix sits in scalar registers)
        const double *m = a.tf + (size_t)r.k * 12;
        ox = (float)(m[0] * (double)x + m[1] * (double)y + m[2] * (double)z + m[3]);
        oy = (float)(m[4] * (double)x + m[5] * (double)y + m[6] * (double)z + m[7]);
        oz = (float)(m[8] * (double)x + m[9] * (double)y + m[10] * (double)z + m[11]);
    }
    float *o = a.out + (size_t)at * CPS_F;
    o[0] = ox; o[1] = oy; o[2] = oz; o[3] = p[3]; o[4] = (float)a.lag[r.k];
}

}  // namespace md

using namespace md;

// workgroups of the count and scatter kernels of md_cp_sweeps_merge: one per 256 input rows and one per segment, at least one
static Sz cps_blocks(Sz N, Sz B, Sz S) {
    const Sz nb = (N + 255) / 256 + B * S;
    return nb ? nb : Sz(1);
}
// scratch of md_cp_sweeps_merge: bsum[blocks + 1] i32
extern "C" int64_t md_cp_sweeps_merge_workspace_bytes(int64_t N, int64_t B, int64_t S) {
    return any_negative({N, B, S}) ? -1 : ws_answer((int64_t)((cps_blocks(N, B, S) + 1) * 4));
}

extern "C" int md_cp_sweeps_merge(MD_AOT_ARGS) {
    // in : points[N,Fin] f32, seg_range[B,S,2] i32, transforms[B,S,12] f64, time_lag[B,S] f64, seg_flags[B,S] i32
    // out: points_out[M,5] f32, offsets_out[B+1] i32, status[B] i32 ; [workspace]
    Args a(MD_ARGS, 8, 9);
    const md_cp_sweeps_attrs *at = a.attrs<md_cp_sweeps_attrs>(extra);
    a.tensor(0, F32, 2); a.tensor(1, I32, 3); a.tensor(2, "float64", 3); a.tensor(3, "float64", 2); a.tensor(4, I32, 2);
    a.tensor(5, F32, 2); a.tensor(6, I32, 1); a.tensor(7, I32, 1); a.scratch(8);
    if (int rc = a.rc()) return rc;
    const int64_t N = a.d(0, 0), Fin = a.d(0, 1), B = a.d(1, 0), S = a.d(1, 1), M = a.d(5, 0);
    a.require(N >= 0 && (Fin == 4 || Fin == 5) && B >= 0 && S >= 0 && a.d(1, 2) == 2);
    a.require(a.d(2, 0) == B && a.d(2, 1) == S && a.d(2, 2) == 12 && a.d(3, 0) == B && a.d(3, 1) == S && a.same_shape(4, 3));
    a.require(M >= N && a.d(5, 1) == CPS_F && a.d(6, 0) == B + 1 && a.d(7, 0) == B);
    a.require(at->reserved0 == 0 && isfinite(at->radius) && at->radius >= 0.f);
    if (int rc = a.rc()) return rc;
    if (N >= ((int64_t)1 << 30) || M >= ((int64_t)1 << 30) || S > CPS_MAX_SWEEPS || B > CPS_MAX_BATCH) return MD_ERR_SIZE;
    if (!a.have({6})) return MD_ERR_ARG;
    if (B > 0 && !a.have({7})) return MD_ERR_ARG;
    if (B * S > 0 && !a.have({1, 2, 3, 4})) return MD_ERR_ARG;
    if (N > 0 && !a.have({0})) return MD_ERR_ARG;
    if (M > 0 && !a.have({5})) return MD_ERR_ARG;
    if (aliased(params, 5, 8)) return MD_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (int64_t)cps_blocks(N, B, S);
    Scratch ws;
    if (int rc = ws.acquire((size_t)md_cp_sweeps_merge_workspace_bytes(N, B, S), a, 8, s)) return rc;
    SweepArgs k;
    k.pts = (const float *)params[0]; k.range = (const int *)params[1]; k.tf = (const double *)params[2];
    k.lag = (const double *)params[3]; k.flags = (const int *)params[4];
    k.out = (float *)params[5]; k.offsets_out = (int *)params[6]; k.status = (int *)params[7]; k.bsum = (int *)ws.ptr;
    k.N = (int)N; k.Fin = (int)Fin; k.M = (int)M; k.B = (int)B; k.S = (int)S; k.nb = (int)nb; k.radius = at->radius;
    hipLaunchKernelGGL(cps_count_kernel, dim3((unsigned)nb), dim3(256), 0, s, k);
    hipLaunchKernelGGL(cps_scan_kernel, dim3(1), dim3(256), 0, s, k);
    hipLaunchKernelGGL(cps_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, s, k);
    return launched();
}
