// cnloss.hip -- CenterNet training loss on the device (include/minddet_hip_cn.h; the consumer of cntargets.hip's outputs).
//
// What it replaces: CenterNetLossCell.construct behind the network (minddet/models/centernet/src/centernet_det.py:177-237) with the
// Sigmoid cell (:168-169), FocalLoss and RegLoss (src/utils.py:48-245): a sigmoid, a clip, two logs and three pows over every (cell,
// class), two transposes and gathers and half a dozen reductions as framework ops, and the same again backwards.
// Three launches and no host read, memset or floating-point atomic:
//   cn_loss_count_kernel   workgroups [0, chunks): the cells with hm == 1 in a chunk of 16384 heat-map elements, an integer, in the
//                          workspace; workgroups [chunks, chunks + B): one sample's valid slots and its two sums of |pred - target|
//   cn_loss_dense_kernel   one workgroup per strip of 64 cells of one sample: num_pos from the chunk counts (a sum of integers: any order
//                          gives the same value), the strip's head rows staged in LDS by contiguous 16-byte loads, the target planes
//                          read with lane = x, the focal term and its derivative per (cell, class); the grad strip (every channel:
//                          zeros for the regression and padding channels) is assembled in LDS and stored contiguously; leaves the
//                          strip's (pos, neg) as float64 in the workspace
//   cn_loss_finish_kernel  workgroup 0 reduces the partials in a fixed order into parts / num_pos / total; with the gradient, workgroup b
//                          writes the regression elements that sample b's slots touch: of the slots sharing a cell the first sums its
//                          siblings' signs and stores each element once
// Arithmetic: every term and every sum in float64, rounded to fp32 once on output (the header says why).
// The block sums and their order, the focal terms, the strip staging, the L1 slot pieces and the entry's ownership rule: loss_common.h.
#include "loss_common.h"
#include "../../include/minddet_hip_cn.h"

#pragma clang fp contract(off)

namespace md {

static_assert(sizeof(md_cn_loss_attrs) == 4 * 4 + 3 * 4, "minddet_hip_cn.h: attribute struct layout");

constexpr int CNL_STRIP = MD_CN_LOSS_STRIP;
constexpr int CNL_CHUNK = MD_CN_LOSS_COUNT_CHUNK;
constexpr int CNL_MAX_M = MD_CN_MAX_OBJS;
constexpr int CNL_REC = 4;             // doubles per sample in the workspace: valid slots, sum |wh|, sum |off|, unused
constexpr int CNL_LDS_HEAD = 96;       // bytes in front of the staged strip: red[4][2], N, cnt[4] (rounded up to a multiple of 16)

struct CnlParams {
    int B, C, HW, Cp, M, strips_per_sample, n_chunks;
    int off_hm, off_wh, off_reg, use_off;
    long long hm_elems;
    float hm_weight, wh_weight, off_weight;
};

__global__ __launch_bounds__(256) void cn_loss_count_kernel(const uint16_t *__restrict__ head, const float *__restrict__ hm,
                                                            const int *__restrict__ ind, const uint8_t *__restrict__ mask,
                                                            const float *__restrict__ wh, const float *__restrict__ reg, CnlParams p,
                                                            int vec, int *__restrict__ counts, double *__restrict__ rec) {
    __shared__ int ired[4];
    __shared__ double red[4 * 3];
    if ((int)blockIdx.x < p.n_chunks) {
        const long long c0 = (long long)blockIdx.x * CNL_CHUNK;
        const int n = (int)min((long long)CNL_CHUNK, p.hm_elems - c0);
        const float *src = hm + c0;
        int cnt = 0;
        if (vec) {   // hm 16-byte aligned: so is every chunk
            for (int i = threadIdx.x; i < n / 4; i += 256) {
                const float4 v = ((const float4 *)src)[i];
                cnt += (v.x == 1.f) + (v.y == 1.f) + (v.z == 1.f) + (v.w == 1.f);
            }
            for (int i = (n & ~3) + threadIdx.x; i < n; i += 256) cnt += src[i] == 1.f;
        } else {
            for (int i = threadIdx.x; i < n; i += 256) cnt += src[i] == 1.f;
        }
        cnt = block_count(cnt, ired);
        if (threadIdx.x == 0) counts[blockIdx.x] = cnt;
        return;
    }
    const int b = blockIdx.x - p.n_chunks;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < p.M; k += 256) {
        const size_t s = (size_t)b * p.M + k;
        const int i = ind[s];
        if (!slot_valid(mask[s], i, p.HW)) continue;
        const uint16_t *cell = head + ((size_t)b * p.HW + i) * p.Cp;
        acc[0] += 1.0;
        acc[1] += fabs((double)bf2f(cell[p.off_wh]) - (double)wh[s * 2]) + fabs((double)bf2f(cell[p.off_wh + 1]) - (double)wh[s * 2 + 1]);
        if (p.use_off)
            acc[2] += fabs((double)bf2f(cell[p.off_reg]) - (double)reg[s * 2]) + fabs((double)bf2f(cell[p.off_reg + 1]) - (double)reg[s * 2 + 1]);
    }
    block_sums<3>(acc, red);
    if (threadIdx.x == 0) {
        double *dst = rec + (size_t)b * CNL_REC;
        dst[0] = acc[0]; dst[1] = acc[1]; dst[2] = acc[2]; dst[3] = 0.0;
    }
}

template <bool GRAD>
__global__ __launch_bounds__(256) void cn_loss_dense_kernel(const uint16_t *__restrict__ head, const float *__restrict__ hm, CnlParams p,
                                                            int vec, const int *__restrict__ counts, double *__restrict__ part,
                                                            float *__restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *red = (double *)smem;                   // [4][2]
    double *s_n = red + 8;                          // [1]: N
    int *ired = (int *)(s_n + 1);                   // [4]
    uint16_t *sh = (uint16_t *)(smem + CNL_LDS_HEAD);                            // [CNL_STRIP][Cp] bf16
    float *sg = (float *)(smem + CNL_LDS_HEAD + (size_t)CNL_STRIP * p.Cp * 2);   // [CNL_STRIP][Cp] f32 (GRAD)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Strip st = strip_of_block(p.strips_per_sample, CNL_STRIP, p.HW, p.Cp);
    const int b = st.b, n0 = st.n0, cells = st.cells;

    stage_strip<GRAD>(sh, sg, head + st.base, st.elems, vec);
    {   // num_pos: a sum of exact integers
        int n = 0;
        for (int i = threadIdx.x; i < p.n_chunks; i += 256) n += counts[i];
        n = block_count(n, ired);   // (the barriers inside also publish sh / sg)
        if (threadIdx.x == 0) s_n[0] = n > 0 ? (double)n : 1.0;
    }
    __syncthreads();

    const double scale = -(double)p.hm_weight / s_n[0];
    double acc[2] = {0.0, 0.0};   // pos, neg of this lane
    if (lane < cells) {
        const float *plane = hm + (size_t)b * p.C * p.HW + n0 + lane;
        for (int c = wave; c < p.C; c += 4) {   // one wave per class row of the strip, lane = cell
            const float t = plane[(size_t)c * p.HW];
            const bool is_pos = t == 1.f, is_neg = t < 1.f;
            if (!is_pos && !is_neg) continue;   // hm > 1 or NaN: in neither sum (the grad strip is already zero)
            bool open;
            const double pr = clipped_p(bf2f(sh[lane * p.Cp + p.off_hm + c]), open);
            double d;
            if (is_pos) {
                acc[0] += pos_term(pr);
                d = pos_term_grad(pr, open);
            } else {
                acc[1] += neg_term(pr, t);
                d = neg_term_grad(pr, open, t);
            }
            if (GRAD) {
                const float g = open ? (float)(scale * d) : 0.f;
                sg[lane * p.Cp + p.off_hm + c] = g == 0.f ? 0.f : g;   // (+0 also where hm_weight is 0)
            }
        }
    }
    block_sums<2>(acc, red);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.x * 2] = acc[0];
        part[(size_t)blockIdx.x * 2 + 1] = acc[1];
    }
    if (GRAD) flush_strip(grad + st.base, sg, st.elems, vec);   // (the block sums' barriers stand between the last write of sg and these reads)
}

template <bool GRAD>
__global__ __launch_bounds__(256) void cn_loss_finish_kernel(const uint16_t *__restrict__ head, const int *__restrict__ ind,
                                                             const uint8_t *__restrict__ mask, const float *__restrict__ wh,
                                                             const float *__restrict__ reg, CnlParams p, const int *__restrict__ counts,
                                                             const double *__restrict__ rec, const double *__restrict__ part,
                                                             int n_strips, float *__restrict__ parts, float *__restrict__ num_pos,
                                                             float *__restrict__ total, float *__restrict__ grad) {
    __shared__ double red[4 * 6];
    __shared__ int s_ind[GRAD ? CNL_MAX_M : 1];
    const int b = blockIdx.x;
    // the batch's valid slots: a sum of exact integers (every workgroup needs it for the regression gradient)
    double nv[1] = {0.0};
    for (int i = threadIdx.x; i < p.B; i += 256) nv[0] += rec[(size_t)i * CNL_REC];
    block_sums<1>(nv, red);
    const double den = 2.0 * nv[0] + 1e-4;
    if (b == 0) {
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // num_pos, sum |wh|, sum |off|, pos, neg, -
        for (int i = threadIdx.x; i < p.n_chunks; i += 256) acc[0] += (double)counts[i];
        for (int i = threadIdx.x; i < p.B; i += 256) {
            acc[1] += rec[(size_t)i * CNL_REC + 1];
            acc[2] += rec[(size_t)i * CNL_REC + 2];
        }
        for (int i = threadIdx.x; i < n_strips; i += 256) {
            acc[3] += part[(size_t)i * 2];
            acc[4] += part[(size_t)i * 2 + 1];
        }
        block_sums<6>(acc, red);
        if (threadIdx.x == 0) {
            const double n = acc[0] == 0.0 ? 1.0 : acc[0];
            const double hm_loss = -(acc[3] + acc[4]) / n, wh_loss = acc[1] / den, off_loss = p.use_off ? acc[2] / den : 0.0;
            parts[0] = (float)hm_loss;
            parts[1] = (float)wh_loss;
            parts[2] = (float)off_loss;
            num_pos[0] = (float)acc[0];
            total[0] = (float)(((double)p.hm_weight * hm_loss + (double)p.wh_weight * wh_loss) + (double)p.off_weight * off_loss);
        }
    }
    if (!GRAD) return;

    const size_t row0 = (size_t)b * p.M;
    for (int k = threadIdx.x; k < p.M; k += 256) {
        const int i = ind[row0 + k];
        s_ind[k] = slot_valid(mask[row0 + k], i, p.HW) ? i : -1;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < p.M; k += 256) {
        const int i = s_ind[k];
        if (i < 0) continue;
        bool owner = true;   // no earlier valid slot on this cell
        for (int k2 = 0; k2 < k; ++k2) owner = owner && s_ind[k2] != i;
        if (!owner) continue;
        const size_t cell_at = ((size_t)b * p.HW + i) * p.Cp;
        const uint16_t *cell = head + cell_at;
        const float pw0 = bf2f(cell[p.off_wh]), pw1 = bf2f(cell[p.off_wh + 1]);
        const float po0 = p.use_off ? bf2f(cell[p.off_reg]) : 0.f, po1 = p.use_off ? bf2f(cell[p.off_reg + 1]) : 0.f;
        int sw0 = 0, sw1 = 0, so0 = 0, so1 = 0;
        for (int k2 = k; k2 < p.M; ++k2) {
            if (s_ind[k2] != i) continue;
            const float *tw = wh + (row0 + k2) * 2;
            sw0 += l1_sign(pw0, tw[0]);
            sw1 += l1_sign(pw1, tw[1]);
            if (p.use_off) {
                const float *tr = reg + (row0 + k2) * 2;
                so0 += l1_sign(po0, tr[0]);
                so1 += l1_sign(po1, tr[1]);
            }
        }
        grad[cell_at + p.off_wh] = reg_grad(p.wh_weight, sw0, den);
        grad[cell_at + p.off_wh + 1] = reg_grad(p.wh_weight, sw1, den);
        if (p.use_off) {
            grad[cell_at + p.off_reg] = reg_grad(p.off_weight, so0, den);
            grad[cell_at + p.off_reg + 1] = reg_grad(p.off_weight, so1, den);
        }
    }
}

// scratch of md_cn_loss and md_cn_loss_grad: rec[B][CNL_REC] f64 at 0, part[B sps][2] f64, counts[chunks] i32; sps = the strips of
// CNL_STRIP cells per sample, chunks = the chunks of CNL_CHUNK heat-map elements of the batch
struct CnlScratch { int64_t sps, chunks, part, counts, total; };
static CnlScratch cn_loss_scratch(Sz B, Sz C, Sz H, Sz W) {
    const Sz sps = (H * W + (CNL_STRIP - 1)) / CNL_STRIP, chunks = (B * C * H * W + (CNL_CHUNK - 1)) / CNL_CHUNK;
    const Sz part = 8 * CNL_REC * B, counts = part + 8 * 2 * B * sps, total = counts + 4 * chunks;
    return {(int64_t)sps, (int64_t)chunks, (int64_t)part, (int64_t)counts, (int64_t)total};
}

static int cn_loss_entry(MD_AOT_ARGS, bool with_grad) {
    // in : head[B,H,W,Cp] bf16, hm[B,C,H,W] f32, ind[B,M] i32, reg_mask[B,M] u8, wh[B,M,2] f32, reg[B,M,2] f32
    // out: parts[3] f32, num_pos[1] f32, total[1] f32 [, grad[B,H,W,Cp] f32] ; [workspace]
    const int n_out = with_grad ? 4 : 3, WS = 6 + n_out;
    Args a(MD_ARGS, WS, WS + 1);
    const md_cn_loss_attrs *at = a.attrs<md_cn_loss_attrs>(extra);
    a.tensor(0, BF16, 4); a.tensor(1, F32, 4); a.tensor(2, I32, 2); a.tensor(3, U8, 2); a.tensor(4, F32, 3); a.tensor(5, F32, 3);
    a.tensor(6, F32, 1); a.tensor(7, F32, 1); a.tensor(8, F32, 1);
    if (with_grad) a.tensor(9, F32, 4);
    a.scratch(WS);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), H = a.d(0, 1), W = a.d(0, 2), Cp = a.d(0, 3), C = a.d(1, 1), M = a.d(2, 1);
    a.require(B >= 1 && H >= 1 && W >= 1 && Cp >= 1 && C >= 1 && M >= 0);
    a.require(a.d(1, 0) == B && a.d(1, 2) == H && a.d(1, 3) == W && a.d(2, 0) == B && a.d(3, 0) == B && a.d(3, 1) == M);
    for (int i = 4; i <= 5; ++i) a.require(a.d(i, 0) == B && a.d(i, 1) == M && a.d(i, 2) == 2);
    a.require(a.d(6, 0) == 3 && a.d(7, 0) == 1 && a.d(8, 0) == 1);
    if (with_grad) a.require(a.same_shape(9, 0));
    a.require(at->num_classes == C && at->off_reg >= -1);
    if (int rc = a.rc()) return rc;
    const bool has_reg = at->off_reg != -1;
    const int64_t lo[3] = {at->off_hm, at->off_wh, at->off_reg}, hi[3] = {at->off_hm + C, (int64_t)at->off_wh + 2, (int64_t)at->off_reg + 2};
    heads_disjoint(a, lo, hi, has_reg ? 3 : 2, Cp);
    a.require(isfinite(at->hm_weight) && isfinite(at->wh_weight) && isfinite(at->off_weight));
    if (int rc = a.rc()) return rc;
    const int64_t lim = (int64_t)1 << 30;
    if (M > CNL_MAX_M || Cp > MD_CN_LOSS_MAX_CHANNELS || B > 65535 || a.numel(0) >= lim || a.numel(1) >= lim ||
        mul({B, M, 2}) >= lim)
        return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8}) || (with_grad && !a.have({9}))) return MD_ERR_ARG;
    const CnlScratch w = cn_loss_scratch(B, C, H, W);
    const int64_t HW = H * W, sps = w.sps, n_strips = B * sps, hm_elems = B * C * HW, n_chunks = w.chunks;
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = ws.acquire((size_t)w.total, a, WS, s)) return rc;
    if ((uintptr_t)ws.ptr % 8 != 0) return MD_ERR_ARG;

    CnlParams p;
    memset(&p, 0, sizeof(p));
    p.B = (int)B; p.C = (int)C; p.HW = (int)HW; p.Cp = (int)Cp; p.M = (int)M; p.strips_per_sample = (int)sps; p.n_chunks = (int)n_chunks;
    p.off_hm = at->off_hm; p.off_wh = at->off_wh; p.off_reg = at->off_reg;
    p.use_off = has_reg && at->off_weight > 0.f;
    p.hm_elems = hm_elems;
    p.hm_weight = at->hm_weight; p.wh_weight = at->wh_weight; p.off_weight = at->off_weight;
    double *rec = (double *)ws.ptr, *part = (double *)((char *)ws.ptr + w.part);
    int *counts = (int *)((char *)ws.ptr + w.counts);
    const uint16_t *head = (const uint16_t *)params[0];
    const float *hm = (const float *)params[1], *wh = (const float *)params[4], *reg = (const float *)params[5];
    const int *ind = (const int *)params[2];
    const uint8_t *mask = (const uint8_t *)params[3];
    float *grad = with_grad ? (float *)params[9] : nullptr;
    const int vec = strip_vec(Cp, head, grad), hm_vec = (uintptr_t)hm % 16 == 0;
    const size_t lds = strip_lds_bytes(CNL_LDS_HEAD, CNL_STRIP, Cp, with_grad);   // Cp <= 160: at most 96 + 61440 bytes
    hipLaunchKernelGGL(cn_loss_count_kernel, dim3((unsigned)(n_chunks + B)), dim3(256), 0, s, head, hm, ind, mask, wh, reg, p, hm_vec, counts,
                       rec);
    grad_or_not(with_grad, [&](auto g) {   // the forward alone needs workgroup 0 of the finish kernel only
        constexpr bool GRAD = decltype(g)::value;
        hipLaunchKernelGGL(cn_loss_dense_kernel<GRAD>, dim3((unsigned)n_strips), dim3(256), lds, s, head, hm, p, vec, counts, part, grad);
        hipLaunchKernelGGL(cn_loss_finish_kernel<GRAD>, dim3(GRAD ? (unsigned)B : 1u), dim3(256), 0, s, head, ind, mask, wh, reg, p, counts, rec,
                           part, (int)n_strips, (float *)params[6], (float *)params[7], (float *)params[8], grad);
    });
    return launched();
}

}  // namespace md

using namespace md;

extern "C" int64_t md_cn_loss_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W) {
    return any_negative({B, C, H, W}) ? -1 : ws_answer(cn_loss_scratch(B, C, H, W).total);
}
extern "C" int md_cn_loss(MD_AOT_ARGS) { return cn_loss_entry(nparam, params, ndims, shapes, dtypes, stream, extra, false); }
extern "C" int md_cn_loss_grad(MD_AOT_ARGS) { return cn_loss_entry(nparam, params, ndims, shapes, dtypes, stream, extra, true); }
