// cploss.hip -- CenterPoint training loss on the device (include/minddet_hip_cploss.h; the consumer of cptargets.hip's outputs).
//
// What it replaces: CenterHead.loss (minddet/models/centerpoint/det3d_ms/models/bbox_heads/center_head.py:208-271) with FastFocalLoss
// and RegLoss (det3d_ms/models/losses/centernet_loss.py:22-82): per task a channel slice, sigmoid, clip, two pows, a log, two gathers
// and a handful of reductions as framework ops, and the same again backwards.  Three launches and no host read, memset or atomic:
//   cp_loss_slot_kernel    one workgroup per (task, sample): per valid slot the positive focal term and the ten |pred - target|, summed
//                          in a fixed order; leaves (valid count, pos, l1[10]) per (sample, task) in the workspace
//   cp_loss_dense_kernel   one workgroup per strip of 64 cells: the strip's head rows staged in LDS by contiguous 16-byte loads, the
//                          target planes read with lane = x, the negative focal term and its derivative per (cell, class); the grad
//                          strip (every channel: zeros for the regression and padding channels) is assembled in LDS and stored
//                          contiguously; leaves one float64 partial per (strip, task) in the workspace
//   cp_loss_finish_kernel  workgroup (0, 0) reduces the partials in a fixed order, one wave per task, into parts / num_pos / total; with
//                          the gradient, workgroup (task, sample) writes the elements that slots touch: of the slots sharing a cell
//                          (and class) the first sums its siblings in slot order and stores the element once, from the float64 sum
// Arithmetic: every term and every sum in float64, rounded to fp32 once on output (the header says why).
// The block sums and their order, the focal terms, the strip staging and the entry's ownership rule: loss_common.h.
#include "loss_common.h"
#include "../../include/minddet_hip_cploss.h"

#pragma clang fp contract(off)

namespace md {

static_assert(sizeof(md_cp_loss_attrs) == 4 + MD_CP_MAX_TASKS * 8 * 4 + 4 + 10 * 4, "minddet_hip_cploss.h: attribute struct layout");

constexpr int CPL_STRIP = MD_CP_LOSS_STRIP;
constexpr int CPL_MAX_M = MD_CP_LOSS_MAX_OBJS;
constexpr int CPL_REC = 12;            // doubles per (sample, task) in the workspace: valid count, pos, l1[10]
constexpr int CPL_LDS_HEAD = 4 * 8 * 8 + 8 * 8;   // bytes in front of the staged strip: tacc[4][8], scale[8] (a multiple of 16)

struct CplTask {
    int ncol;                          // 10, or 8 without vel
    int ch[10], tcol[10];              // column j of box_loss: its head channel and its column of anno_box
    int off_hm, nc;
};
struct CplParams {
    int B, T, C, HW, Cp, M, strips_per_sample;
    float weight, cw[10];
    CplTask task[MD_CP_MAX_TASKS];
};

__device__ __forceinline__ bool slot_valid(int m, int i, int c, int HW, int nc) { return slot_valid(m, i, HW) && c >= 0 && c < nc; }

__global__ __launch_bounds__(256) void cp_loss_slot_kernel(const uint16_t *__restrict__ head, const float *__restrict__ anno,
                                                           const int *__restrict__ ind, const uint8_t *__restrict__ mask,
                                                           const int *__restrict__ cat, CplParams p, double *__restrict__ rec) {
    __shared__ double red[4 * CPL_REC];
    const int t = blockIdx.x, b = blockIdx.y;
    const CplTask &tk = p.task[t];
    const size_t row0 = ((size_t)b * p.T + t) * p.M;
    double acc[CPL_REC];
#pragma unroll
    for (int e = 0; e < CPL_REC; ++e) acc[e] = 0.0;
    for (int k = threadIdx.x; k < p.M; k += 256) {
        const int i = ind[row0 + k], c = cat[row0 + k];
        if (!slot_valid(mask[row0 + k], i, c, p.HW, tk.nc)) continue;
        const uint16_t *cell = head + ((size_t)b * p.HW + i) * p.Cp;
        bool open;
        const double pr = clipped_p(bf2f(cell[tk.off_hm + c]), open);
        acc[0] += 1.0;
        acc[1] += pos_term(pr);
        const float *target = anno + (row0 + k) * 10;
#pragma unroll
        for (int j = 0; j < 10; ++j)
            if (j < tk.ncol) acc[2 + j] += fabs((double)bf2f(cell[tk.ch[j]]) - (double)target[tk.tcol[j]]);
    }
    block_sums<CPL_REC>(acc, red);
    if (threadIdx.x == 0) {
        double *dst = rec + ((size_t)b * p.T + t) * CPL_REC;
#pragma unroll
        for (int e = 0; e < CPL_REC; ++e) dst[e] = acc[e];
    }
}

// the valid slots of task t over the batch: a sum of exact integers, so any order gives the same value
__device__ __forceinline__ double wave_num_pos(const double *rec, int t, int B, int T, int lane) {
    double n = 0.0;
    for (int b = lane; b < B; b += 64) n += rec[((size_t)b * T + t) * CPL_REC];
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    return n;
}

template <bool GRAD>
__global__ __launch_bounds__(256) void cp_loss_dense_kernel(const uint16_t *__restrict__ head, const float *__restrict__ hm, CplParams p,
                                                            int vec, const double *__restrict__ rec, double *__restrict__ neg_part,
                                                            float *__restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *tacc = (double *)smem;                  // [4][8]: per wave and task, the negative terms of the strip
    double *scale = tacc + 32;                      // [8]
    uint16_t *sh = (uint16_t *)(smem + CPL_LDS_HEAD);                            // [CPL_STRIP][Cp] bf16
    float *sg = (float *)(smem + CPL_LDS_HEAD + (size_t)CPL_STRIP * p.Cp * 2);   // [CPL_STRIP][Cp] f32 (GRAD)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Strip st = strip_of_block(p.strips_per_sample, CPL_STRIP, p.HW, p.Cp);
    const int b = st.b, n0 = st.n0, cells = st.cells;

    stage_strip<GRAD>(sh, sg, head + st.base, st.elems, vec);
    if (threadIdx.x < 32) tacc[threadIdx.x] = 0.0;
    for (int t = wave; t < p.T; t += 4) {
        const double n = wave_num_pos(rec, t, p.B, p.T, lane);
        if (lane == 0) scale[t] = n > 0.0 ? -1.0 / n : -1.0;
    }
    __syncthreads();

    // one wave per (task, class) row of the strip, lane = cell
    int row = 0;
    for (int t = 0; t < p.T; ++t) {
        const int nc = p.task[t].nc, off_hm = p.task[t].off_hm;
        for (int c = 0; c < nc; ++c, ++row) {
            if ((row & 3) != wave) continue;
            double loss = 0.0, dloss = 0.0;
            if (lane < cells) {
                bool open;
                const double pr = clipped_p(bf2f(sh[lane * p.Cp + off_hm + c]), open);
                const float hmv = hm[(((size_t)b * p.T + t) * p.C + c) * p.HW + n0 + lane];
                loss = neg_term(pr, hmv);
                dloss = neg_term_grad(pr, open, hmv);
                if (GRAD) sg[lane * p.Cp + off_hm + c] = (float)(scale[t] * dloss);
            }
            for (int off = 32; off > 0; off >>= 1) loss += __shfl_down(loss, off, 64);
            if (lane == 0) tacc[wave * 8 + t] += loss;
        }
    }
    __syncthreads();
    if (threadIdx.x < p.T) {
        const int t = threadIdx.x;
        neg_part[(size_t)blockIdx.x * p.T + t] = ((tacc[t] + tacc[8 + t]) + tacc[16 + t]) + tacc[24 + t];
    }
    if (GRAD) flush_strip(grad + st.base, sg, st.elems, vec);
}

template <bool GRAD>
__global__ __launch_bounds__(512) void cp_loss_finish_kernel(const uint16_t *__restrict__ head, const float *__restrict__ hm,
                                                             const float *__restrict__ anno, const int *__restrict__ ind,
                                                             const uint8_t *__restrict__ mask, const int *__restrict__ cat, CplParams p,
                                                             const double *__restrict__ rec, const double *__restrict__ neg_part,
                                                             int n_strips, float *__restrict__ parts, float *__restrict__ num_pos,
                                                             float *__restrict__ total, float *__restrict__ grad) {
    __shared__ double task_loss[MD_CP_MAX_TASKS];
    __shared__ __attribute__((aligned(16))) int s_ind[GRAD ? CPL_MAX_M : 4], s_cat[GRAD ? CPL_MAX_M : 4];
    const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (t == 0 && b == 0) {
        // one wave per task (eight waves, at most eight tasks): lane-strided sums in a fixed order, then the wave's tree
        if (wave < p.T) {
            const int tt = wave;
            double acc[CPL_REC + 1];   // count, pos, l1[10], neg
#pragma unroll
            for (int e = 0; e <= CPL_REC; ++e) acc[e] = 0.0;
            for (int bb = lane; bb < p.B; bb += 64) {
                const double *src = rec + ((size_t)bb * p.T + tt) * CPL_REC;
#pragma unroll
                for (int e = 0; e < CPL_REC; ++e) acc[e] += src[e];
            }
            for (int i = lane; i < n_strips; i += 64) acc[CPL_REC] += neg_part[(size_t)i * p.T + tt];
#pragma unroll
            for (int e = 0; e <= CPL_REC; ++e)
                for (int off = 32; off > 0; off >>= 1) acc[e] += __shfl_down(acc[e], off, 64);
            if (lane == 0) {
                const double n = acc[0], pos = acc[1], neg = acc[CPL_REC];
                const double hm_loss = n == 0.0 ? -neg : -(pos + neg) / n;
                double loc = 0.0;
#pragma unroll
                for (int j = 0; j < 10; ++j) {
                    const double box = j < p.task[tt].ncol ? acc[2 + j] / (n + 1e-4) : 0.0;
                    loc += box * (double)p.cw[j];
                    parts[tt * 12 + 2 + j] = (float)box;
                }
                parts[tt * 12] = (float)hm_loss;
                parts[tt * 12 + 1] = (float)loc;
                num_pos[tt] = (float)n;
                task_loss[tt] = hm_loss + (double)p.weight * loc;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = 0.0;
            for (int tt = 0; tt < p.T; ++tt) tot += task_loss[tt];
            total[0] = (float)tot;
        }
    }
    if (!GRAD) return;

    const CplTask &tk = p.task[t];
    const size_t row0 = ((size_t)b * p.T + t) * p.M;
    const int M4 = (p.M + 3) & ~3;   // the scan below reads four slots at a time
    for (int k = threadIdx.x; k < M4; k += 512) {
        int i = -1, c = 0;
        if (k < p.M) {
            i = ind[row0 + k];
            c = cat[row0 + k];
            if (!slot_valid(mask[row0 + k], i, c, p.HW, tk.nc)) i = -1;
        }
        s_ind[k] = i;
        s_cat[k] = c;
    }
    const double n = wave_num_pos(rec, t, p.B, p.T, lane);
    const double scale = n > 0.0 ? -1.0 / n : -1.0;
    __syncthreads();
    for (int k = threadIdx.x; k < p.M; k += 512) {
        const int i = s_ind[k];
        if (i < 0) continue;
        const int c = s_cat[k];
        // the valid slots on this cell / on this cell and class: before slot k, and from slot k on (k itself included)
        int before_cell = 0, before_class = 0, after_cell = 0, after_class = 0;
        auto tally = [&](int vi, int vc, int k2) {
            const bool same = vi == i, same_class = same && vc == c, before = k2 < k;
            before_cell += same && before;
            before_class += same_class && before;
            after_cell += same && !before;
            after_class += same_class && !before;
        };
        for (int k2 = 0; k2 < M4; k2 += 4) {   // (one 16-byte LDS read per four slots and array: few dependent reads)
            const int4 qi = *(const int4 *)(s_ind + k2), qc = *(const int4 *)(s_cat + k2);
            tally(qi.x, qc.x, k2);
            tally(qi.y, qc.y, k2 + 1);
            tally(qi.z, qc.z, k2 + 2);
            tally(qi.w, qc.w, k2 + 3);
        }
        if (before_class) continue;   // an earlier slot owns this (cell, class), and so this cell's regression channels too
        const size_t cell_at = ((size_t)b * p.HW + i) * p.Cp;
        const uint16_t *cell = head + cell_at;
        {
            bool open;
            const double pr = clipped_p(bf2f(cell[tk.off_hm + c]), open);
            const float hmv = hm[(((size_t)b * p.T + t) * p.C + c) * p.HW + i];
            const double nd = neg_term_grad(pr, open, hmv), pd = pos_term_grad(pr, open);
            double sum = 0.0;
            for (int r = 0; r < after_class; ++r) sum += pd;   // the siblings' terms are equal (one p): added one by one, in slot order
            grad[cell_at + tk.off_hm + c] = (float)(scale * (nd + sum));
        }
        if (before_cell == 0) {
            int sgn[10];
            float pred[10];
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                sgn[j] = 0;
                pred[j] = j < tk.ncol ? bf2f(cell[tk.ch[j]]) : 0.f;
            }
            for (int k2 = k, seen = 0; k2 < p.M && seen < after_cell; ++k2) {   // (ends at the last sibling: at once for a slot alone on its cell)
                if (s_ind[k2] != i) continue;
                ++seen;
                const float *target = anno + (row0 + k2) * 10;
#pragma unroll
                for (int j = 0; j < 10; ++j) {
                    if (j < tk.ncol) {
                        const float tv = target[tk.tcol[j]];
                        sgn[j] += l1_sign(pred[j], tv);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 10; ++j)
                if (j < tk.ncol) grad[cell_at + tk.ch[j]] = (float)((double)p.weight * (double)p.cw[j] * (double)sgn[j] / (n + 1e-4));
        }
    }
}

// scratch of md_cp_loss and md_cp_loss_grad: rec[B T][CPL_REC] f64 at 0, then neg_part[B T][sps] f64, sps = the strips of CPL_STRIP
// cells per sample
struct CplScratch { int64_t sps, neg_part, total; };
static CplScratch cp_loss_scratch(Sz B, Sz T, Sz H, Sz W) {
    const Sz sps = (H * W + (CPL_STRIP - 1)) / CPL_STRIP, neg_part = 8 * B * T * CPL_REC, total = neg_part + 8 * B * T * sps;
    return {(int64_t)sps, (int64_t)neg_part, (int64_t)total};
}

static int cp_loss_entry(MD_AOT_ARGS, bool with_grad) {
    // in : head[B,H,W,Cp] bf16, hm[B,T,C,H,W] f32, anno_box[B,T,M,10] f32, ind[B,T,M] i32, mask[B,T,M] u8, cat[B,T,M] i32
    // out: parts[T,12] f32, num_pos[T] f32, total[1] f32 [, grad[B,H,W,Cp] f32] ; [workspace]
    const int n_out = with_grad ? 4 : 3, WS = 6 + n_out;
    Args a(MD_ARGS, WS, WS + 1);
    const md_cp_loss_attrs *at = a.attrs<md_cp_loss_attrs>(extra);
    a.tensor(0, BF16, 4); a.tensor(1, F32, 5); a.tensor(2, F32, 4); a.tensor(3, I32, 3); a.tensor(4, U8, 3); a.tensor(5, I32, 3);
    a.tensor(6, F32, 2); a.tensor(7, F32, 1); a.tensor(8, F32, 1);
    if (with_grad) a.tensor(9, F32, 4);
    a.scratch(WS);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), H = a.d(0, 1), W = a.d(0, 2), Cp = a.d(0, 3), T = a.d(1, 1), C = a.d(1, 2), M = a.d(2, 2);
    a.require(B >= 1 && H >= 1 && W >= 1 && Cp >= 1 && M >= 0);
    a.require(a.d(1, 0) == B && a.d(1, 3) == H && a.d(1, 4) == W && a.d(2, 0) == B && a.d(2, 1) == T && a.d(2, 3) == 10);
    for (int i = 3; i <= 5; ++i) a.require(a.d(i, 0) == B && a.d(i, 1) == T && a.d(i, 2) == M);
    a.require(a.d(6, 0) == T && a.d(6, 1) == 12 && a.d(7, 0) == T && a.d(8, 0) == 1);
    if (with_grad) a.require(a.same_shape(9, 0));
    a.require(at->num_tasks >= 1 && at->num_tasks <= MD_CP_MAX_TASKS && at->num_tasks == T);
    if (int rc = a.rc()) return rc;

    CplParams p;
    memset(&p, 0, sizeof(p));
    int max_nc = 0, n_range = 0;
    int64_t lo[MD_CP_MAX_TASKS * 6], hi[MD_CP_MAX_TASKS * 6];   // the channel ranges of every head
    for (int t = 0; t < at->num_tasks; ++t) {
        const md_cp_task_attrs &s = at->task[t];
        CplTask &tk = p.task[t];
        a.require(s.num_classes >= 1 && s.num_classes <= 65535 && s.off_vel >= -1);
        const bool vel = s.off_vel != -1;
        const int64_t first[6] = {s.off_reg, s.off_height, s.off_dim, s.off_rot, s.off_hm, s.off_vel};
        const int64_t width[6] = {2, 1, 3, 2, s.num_classes, 2};
        for (int h = 0; h < (vel ? 6 : 5); ++h) {
            lo[n_range] = first[h];
            hi[n_range++] = first[h] + width[h];
        }
        // anno_box columns: reg 0-1, height 2, dim 3-5, vel 6-7, rot 8-9; without vel the rot columns follow dim (center_head.py:239-250)
        const int chans[10] = {s.off_reg, s.off_reg + 1, s.off_height, s.off_dim, s.off_dim + 1, s.off_dim + 2,
                               vel ? s.off_vel : s.off_rot, vel ? s.off_vel + 1 : s.off_rot + 1, s.off_rot, s.off_rot + 1};
        tk.ncol = vel ? 10 : 8;
        for (int j = 0; j < 10; ++j) {
            tk.ch[j] = j < tk.ncol ? chans[j] : 0;
            tk.tcol[j] = !vel && j >= 6 ? (j < 8 ? j + 2 : 0) : j;
        }
        tk.off_hm = s.off_hm;
        tk.nc = s.num_classes;
        max_nc = s.num_classes > max_nc ? s.num_classes : max_nc;
    }
    heads_disjoint(a, lo, hi, n_range, Cp);
    a.require(C == max_nc && isfinite(at->weight));
    for (int j = 0; j < 10; ++j) a.require(isfinite(at->code_weights[j]));
    if (int rc = a.rc()) return rc;
    const int64_t lim = (int64_t)1 << 30;
    if (M > CPL_MAX_M || Cp > MD_CP_LOSS_MAX_CHANNELS || B > 65535 || a.numel(0) >= lim || a.numel(1) >= lim || a.numel(2) >= lim) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8}) || (with_grad && !a.have({9}))) return MD_ERR_ARG;
    const CplScratch w = cp_loss_scratch(B, T, H, W);
    const int64_t HW = H * W, sps = w.sps, n_strips = B * sps;
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = ws.acquire((size_t)w.total, a, WS, s)) return rc;
    p.B = (int)B; p.T = (int)T; p.C = (int)C; p.HW = (int)HW; p.Cp = (int)Cp; p.M = (int)M; p.strips_per_sample = (int)sps;
    p.weight = at->weight;
    for (int j = 0; j < 10; ++j) p.cw[j] = at->code_weights[j];
    double *rec = (double *)ws.ptr, *neg_part = (double *)((char *)ws.ptr + w.neg_part);
    const uint16_t *head = (const uint16_t *)params[0];
    const float *hm = (const float *)params[1], *anno = (const float *)params[2];
    const int *ind = (const int *)params[3], *cat = (const int *)params[5];
    const uint8_t *mask = (const uint8_t *)params[4];
    float *grad = with_grad ? (float *)params[9] : nullptr;
    const int vec = strip_vec(Cp, head, grad);
    const size_t lds = strip_lds_bytes(CPL_LDS_HEAD, CPL_STRIP, Cp, with_grad);
    hipLaunchKernelGGL(cp_loss_slot_kernel, dim3((unsigned)T, (unsigned)B), dim3(256), 0, s, head, anno, ind, mask, cat, p, rec);
    grad_or_not(with_grad, [&](auto g) {   // the forward alone needs workgroup (0, 0) of the finish kernel only
        constexpr bool GRAD = decltype(g)::value;
        hipLaunchKernelGGL(cp_loss_dense_kernel<GRAD>, dim3((unsigned)n_strips), dim3(256), lds, s, head, hm, p, vec, rec, neg_part, grad);
        hipLaunchKernelGGL(cp_loss_finish_kernel<GRAD>, GRAD ? dim3((unsigned)T, (unsigned)B) : dim3(1, 1), dim3(512), 0, s, head, hm, anno, ind,
                           mask, cat, p, rec, neg_part, (int)n_strips, (float *)params[6], (float *)params[7], (float *)params[8], grad);
    });
    return launched();
}

}  // namespace md

using namespace md;

extern "C" int64_t md_cp_loss_workspace_bytes(int64_t B, int64_t T, int64_t H, int64_t W) {
    return any_negative({B, T, H, W}) ? -1 : ws_answer(cp_loss_scratch(B, T, H, W).total);
}
extern "C" int md_cp_loss(MD_AOT_ARGS) { return cp_loss_entry(nparam, params, ndims, shapes, dtypes, stream, extra, false); }
extern "C" int md_cp_loss_grad(MD_AOT_ARGS) { return cp_loss_entry(nparam, params, ndims, shapes, dtypes, stream, extra, true); }
