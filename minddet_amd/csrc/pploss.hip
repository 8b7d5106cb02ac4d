// pploss.hip -- KITTI PointPillars training loss on the device (include/minddet_hip_pploss.h; the consumer of targets.hip's outputs).
//
// What it replaces: PointPillarsWithLossCell.construct behind the network (minddet/models/pointpillars/src/pointpillars.py:817-872) with
// prepare_loss_weights (:19-43), create_loss (:64-98), add_sin_difference (:101-107), _get_pos_neg_loss (:110-127), get_direction_target
// (:142-164) and the three loss classes of src/core/losses.py:40-191: a one-hot, sigmoid / log1p / exp / pow over every anchor and class,
// sin / cos over every anchor, a softmax cross-entropy and half a dozen reductions as framework ops, and the same again backwards.
// Three launches and no host read, memset or floating-point atomic:
//   pp_loss_count_kernel   one workgroup per chunk of 4096 labels of one sample: the chunk's positives, an integer, in the workspace
//   pp_loss_dense_kernel   one workgroup per strip of 64 cells of one sample: the sample's positive count from the chunk counts (a sum of
//                          integers: any order gives the same value), the strip's head rows staged in LDS by contiguous 16-byte loads and
//                          its labels beside them; the focal term and its derivative per (anchor, class), the smooth-L1 and direction
//                          terms per positive anchor (reg_targets and the anchor's rotation are loaded for these only); the grad strip
//                          (every channel: zeros where nothing is owed) is assembled in LDS and stored contiguously; leaves five float64
//                          partials (loc, cls, dir, cls_pos, cls_neg; already divided by n_b) per strip in the workspace
//   pp_loss_finish_kernel  one workgroup reduces the partials in a fixed order into parts / total and writes num_pos
// Arithmetic: every term and every sum in float64, rounded to fp32 once on output (the header says why).
// The block sums and their order, the strip staging and the entry's ownership rule: loss_common.h.
#include "loss_common.h"
#include "../../include/minddet_hip_pploss.h"

#pragma clang fp contract(off)

namespace md {

static_assert(sizeof(md_pp_loss_attrs) == 7 * 4 + 3 * 4 + 7 * 4 + 3 * 4 + 2 * 4, "minddet_hip_pploss.h: attribute struct layout");

constexpr int PPL_STRIP = MD_PP_LOSS_STRIP;
constexpr int PPL_CHUNK = MD_PP_LOSS_COUNT_CHUNK;
constexpr int PPL_Q = 5;               // doubles per strip in the workspace: loc, cls, dir, cls_pos, cls_neg
constexpr int PPL_LDS_HEAD = 176;      // bytes in front of the staged strip: red[4][5], n_b (rounded up to a multiple of 16)

struct PplParams {
    int B, HW, C, A, K, N, strips_per_sample, chunks_per_sample;
    int off_cls, off_box, off_dir;
    float alpha, gamma, sigma, cw[7], cls_weight, loc_weight, dir_weight, pos_cls_weight, neg_cls_weight;
};

// softplus(s) = max(s, 0) + log1p(exp(-|s|)), m = sigmoid(s) and om = 1 - sigmoid(s) = sigmoid(-s), none of them by a subtraction from 1
__device__ __forceinline__ void softplus_sigmoid(double s, double &sp, double &m, double &om) {
    const double e = exp(-fabs(s)), r = 1.0 / (1.0 + e);
    sp = fmax(s, 0.0) + log1p(e);
    m = s >= 0.0 ? r : e * r;
    om = s >= 0.0 ? e * r : r;
}

__global__ __launch_bounds__(256) void pp_loss_count_kernel(const int *__restrict__ labels, int N, int chunks_per_sample,
                                                            int *__restrict__ counts) {
    __shared__ int red[4];
    const int b = blockIdx.y, c0 = blockIdx.x * PPL_CHUNK;
    const int n = min(PPL_CHUNK, N - c0);
    const int *src = labels + (size_t)b * N + c0;
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += 256) cnt += src[i] > 0;
    cnt = block_count(cnt, red);
    if (threadIdx.x == 0) counts[(size_t)b * chunks_per_sample + blockIdx.x] = cnt;
}

template <bool GRAD>
__global__ __launch_bounds__(256) void pp_loss_dense_kernel(const uint16_t *__restrict__ head, const int *__restrict__ labels,
                                                            const float *__restrict__ reg, const float *__restrict__ anchors, PplParams p,
                                                            int vec, const int *__restrict__ counts, double *__restrict__ part,
                                                            float *__restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *red = (double *)smem;                   // [4][PPL_Q]
    double *s_nb = red + 4 * PPL_Q;                 // [1]: n_b
    int *s_lab = (int *)(smem + PPL_LDS_HEAD);                                              // [PPL_STRIP][A]
    uint16_t *sh = (uint16_t *)(smem + PPL_LDS_HEAD + (size_t)PPL_STRIP * p.A * 4);         // [PPL_STRIP][C] bf16
    float *sg = (float *)(smem + PPL_LDS_HEAD + (size_t)PPL_STRIP * (p.A * 4 + p.C * 2));   // [PPL_STRIP][C] f32 (GRAD)
    const int lane = threadIdx.x & 63;
    const Strip st = strip_of_block(p.strips_per_sample, PPL_STRIP, p.HW, p.C);
    const int b = st.b, n0 = st.n0, nanch = st.cells * p.A;
    const size_t anchor0 = (size_t)b * p.N + (size_t)n0 * p.A;  // of the strip's first anchor in labels and reg_targets

    stage_strip<GRAD>(sh, sg, head + st.base, st.elems, vec);
    for (int i = threadIdx.x; i < nanch; i += 256) s_lab[i] = labels[anchor0 + i];
    if (threadIdx.x < 64) {   // the sample's positives: a sum of exact integers
        int n = 0;
        for (int i = lane; i < p.chunks_per_sample; i += 64) n += counts[(size_t)b * p.chunks_per_sample + i];
        n = wave_sum_all(n);
        if (lane == 0) s_nb[0] = (double)max(n, 1);
    }
    __syncthreads();

    const double nb = s_nb[0], batch = (double)p.B;
    const double w_pos = (double)p.pos_cls_weight / nb, w_neg = (double)p.neg_cls_weight / nb;
    const double a_pos = p.alpha < 0.f ? 1.0 : (double)p.alpha, a_neg = p.alpha < 0.f ? 1.0 : 1.0 - (double)p.alpha;
    const double gamma = (double)p.gamma, g_cls = (double)p.cls_weight / batch;
    double acc[PPL_Q] = {0.0, 0.0, 0.0, 0.0, 0.0};   // loc, cls, dir, cls_pos, cls_neg of this lane, before the division by n_b where it is owed

    // classification: one lane per (anchor, class) of the strip
    for (int e = threadIdx.x; e < nanch * p.K; e += 256) {
        const int na = e / p.K, k = e - na * p.K, cell = na / p.A, a = na - cell * p.A;
        const int lab = s_lab[na];
        if (lab < 0) continue;   // ignored: w = 0, the term and its derivative are exactly 0 (the grad strip is already zero)
        const int ch = cell * p.C + p.off_cls + a * p.K + k;
        const bool z = lab == k + 1;
        const double x = (double)bf2f(sh[ch]), s = z ? -x : x;
        double ce, m, om;
        softplus_sigmoid(s, ce, m, om);
        const double mod = gamma == 0.0 ? 1.0 : (gamma == 2.0 ? m * m : pow(m, gamma));
        const double aw = (z ? a_pos : a_neg) * (lab > 0 ? w_pos : w_neg);
        const double term = mod * aw * ce;
        acc[1] += term;
        if (p.K == 1 ? lab > 0 : k >= 1) acc[3] += term;
        else acc[4] += term;
        if (GRAD) {
            const double d = g_cls * aw * mod * (gamma * om * ce + m);
            sg[ch] = (float)(z ? -d : d);
        }
    }

    // localisation and direction: one lane per positive anchor of the strip
    const double sigma = (double)p.sigma, sigma2 = sigma * sigma, knee = 1.0 / sigma2, g_loc = (double)p.loc_weight / batch / nb,
                 g_dir = (double)p.dir_weight / batch / nb;
    for (int na = threadIdx.x; na < nanch; na += 256) {
        if (s_lab[na] <= 0) continue;
        const int cell = na / p.A, a = na - cell * p.A;
        const float *tgt = reg + (anchor0 + na) * 7;
        const int ch0 = cell * p.C + p.off_box + a * 7;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const double pr = (double)bf2f(sh[ch0 + j]), tg = (double)tgt[j], cw = (double)p.cw[j];
            double d, chain = 1.0;
            if (j < 6) {
                d = cw * (pr - tg);
            } else {
                const double sp = sin(pr), cp = cos(pr), st = sin(tg), ct = cos(tg);
                d = cw * (sp * ct - cp * st);
                chain = cp * ct + sp * st;   // cos(pred - tgt)
            }
            const double ad = fabs(d);
            const bool quad = ad <= knee;
            const double sd = ad * sigma;
            acc[0] += quad ? 0.5 * (sd * sd) : ad - 0.5 / sigma2;
            if (GRAD) {
                const double slope = quad ? sigma2 * d : (d > 0.0 ? 1.0 : -1.0);
                sg[ch0 + j] = (float)(g_loc * cw * slope * chain);
            }
        }
        if (p.off_dir >= 0) {
            const int n = n0 * p.A + na;
            const float rot = tgt[6] + anchors[(size_t)n * 7 + 6];   // the fp32 sum of get_direction_target
            const int t = rot > 0.f ? 1 : 0, cd = cell * p.C + p.off_dir + a * 2;
            const double u = (double)bf2f(sh[cd + 1 - t]) - (double)bf2f(sh[cd + t]);
            double sp, m, om;
            softplus_sigmoid(u, sp, m, om);
            acc[2] += sp;
            if (GRAD) {
                const double d = g_dir * m;
                sg[cd + 1 - t] = (float)d;
                sg[cd + t] = (float)-d;
            }
        }
    }

    block_sums<PPL_Q>(acc, red);
    if (threadIdx.x == 0) {
        double *dst = part + (size_t)blockIdx.x * PPL_Q;
        dst[0] = acc[0] / nb;
        dst[1] = acc[1];
        dst[2] = acc[2] / nb;
        dst[3] = acc[3];
        dst[4] = acc[4];
    }
    if (GRAD) flush_strip(grad + st.base, sg, st.elems, vec);   // (the block sums' barriers stand between the last write of sg and these reads)
}

__global__ __launch_bounds__(256) void pp_loss_finish_kernel(const double *__restrict__ part, const int *__restrict__ counts, PplParams p,
                                                             int n_strips, float *__restrict__ parts, float *__restrict__ num_pos,
                                                             float *__restrict__ total) {
    __shared__ double red[4 * PPL_Q];
    double acc[PPL_Q] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n_strips; i += 256) {
#pragma unroll
        for (int e = 0; e < PPL_Q; ++e) acc[e] += part[(size_t)i * PPL_Q + e];
    }
    block_sums<PPL_Q>(acc, red);
    if (threadIdx.x == 0) {
        const double batch = (double)p.B;
        const double loc = (double)p.loc_weight * acc[0] / batch, cls = (double)p.cls_weight * acc[1] / batch;
        const double dir = p.off_dir >= 0 ? (double)p.dir_weight * acc[2] / batch : 0.0;
        parts[0] = (float)loc;
        parts[1] = (float)cls;
        parts[2] = (float)dir;
        parts[3] = (float)(acc[3] / batch / (double)p.pos_cls_weight);
        parts[4] = (float)(acc[4] / batch / (double)p.neg_cls_weight);
        total[0] = (float)((loc + cls) + dir);
    }
    for (int b = threadIdx.x; b < p.B; b += 256) {
        int n = 0;
        for (int i = 0; i < p.chunks_per_sample; ++i) n += counts[(size_t)b * p.chunks_per_sample + i];
        num_pos[b] = (float)n;
    }
}

// scratch of md_pp_loss and md_pp_loss_grad: part[B sps][PPL_Q] f64 at 0, then counts[B][cps] i32; sps = the strips of PPL_STRIP cells,
// cps = the chunks of PPL_CHUNK labels per sample
struct PplScratch { int64_t sps, cps, counts, total; };
static PplScratch pp_loss_scratch(Sz B, Sz H, Sz W, Sz A) {
    const Sz sps = (H * W + (PPL_STRIP - 1)) / PPL_STRIP, cps = (H * W * A + (PPL_CHUNK - 1)) / PPL_CHUNK;
    const Sz counts = 8 * PPL_Q * B * sps, total = counts + 4 * B * cps;
    return {(int64_t)sps, (int64_t)cps, (int64_t)counts, (int64_t)total};
}

static int pp_loss_entry(MD_AOT_ARGS, bool with_grad) {
    // in : head[B,H,W,C] bf16, labels[B,N] i32, reg_targets[B,N,7] f32, anchors[N,7] f32
    // out: parts[5] f32, num_pos[B] f32, total[1] f32 [, grad[B,H,W,C] f32] ; [workspace]
    const int n_out = with_grad ? 4 : 3, WS = 4 + n_out;
    Args a(MD_ARGS, WS, WS + 1);
    const md_pp_loss_attrs *at = a.attrs<md_pp_loss_attrs>(extra);
    a.tensor(0, BF16, 4); a.tensor(1, I32, 2); a.tensor(2, F32, 3); a.tensor(3, F32, 2);
    a.tensor(4, F32, 1); a.tensor(5, F32, 1); a.tensor(6, F32, 1);
    if (with_grad) a.tensor(7, F32, 4);
    a.scratch(WS);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), H = a.d(0, 1), W = a.d(0, 2), C = a.d(0, 3);
    const md_pp_head_attrs &h = at->head;
    a.require(B >= 1 && H >= 1 && W >= 1 && C >= 1);
    a.require(h.num_anchors >= 1 && h.num_classes >= 1 && h.score_mode == 0 && h.self_train == 1 && h.off_dir >= -1);
    if (int rc = a.rc()) return rc;
    const int64_t A = h.num_anchors, K = h.num_classes, HW = H * W;
    // (A K <= C, so the products below are small)
    const bool dir = h.off_dir != -1;
    const int64_t lo[3] = {h.off_cls, h.off_box, h.off_dir}, hi[3] = {h.off_cls + A * K, h.off_box + A * 7, h.off_dir + A * 2};
    a.require(A <= C && K <= C);
    heads_disjoint(a, lo, hi, dir ? 3 : 2, C);
    if (int rc = a.rc()) return rc;
    const int64_t lim = (int64_t)1 << 30;
    const bool big = B >= lim || HW >= lim || mul({HW, A}) >= lim;   // N itself past the limit: the extents below cannot be compared safely
    const int64_t N = big ? 0 : HW * A;
    if (!big) {
        a.require(a.d(1, 0) == B && a.d(1, 1) == N && a.d(2, 0) == B && a.d(2, 1) == N && a.d(2, 2) == 7 && a.d(3, 0) == N && a.d(3, 1) == 7);
        a.require(a.d(4, 0) == 5 && a.d(5, 0) == B && a.d(6, 0) == 1);
        if (with_grad) a.require(a.same_shape(7, 0));
    }
    const float fl[] = {at->alpha, at->gamma, at->sigma, at->cls_weight, at->loc_weight, at->dir_weight, at->pos_cls_weight, at->neg_cls_weight};
    for (float v : fl) a.require(isfinite(v));
    for (int j = 0; j < 7; ++j) a.require(isfinite(at->code_weights[j]));
    a.require(at->gamma >= 0.f && at->sigma > 0.f && at->pos_cls_weight > 0.f && at->neg_cls_weight > 0.f);
    if (int rc = a.rc()) return rc;
    if (big || C > MD_PP_LOSS_MAX_CHANNELS || B > 65535 || a.numel(0) >= lim || a.numel(2) >= lim) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6}) || (with_grad && !a.have({7}))) return MD_ERR_ARG;
    const PplScratch w = pp_loss_scratch(B, H, W, A);
    const int64_t sps = w.sps, n_strips = B * sps, cps = w.cps;
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = ws.acquire((size_t)w.total, a, WS, s)) return rc;
    if ((uintptr_t)ws.ptr % 8 != 0) return MD_ERR_ARG;

    PplParams p;
    memset(&p, 0, sizeof(p));
    p.B = (int)B; p.HW = (int)HW; p.C = (int)C; p.A = (int)A; p.K = (int)K; p.N = (int)N;
    p.strips_per_sample = (int)sps; p.chunks_per_sample = (int)cps;
    p.off_cls = h.off_cls; p.off_box = h.off_box; p.off_dir = h.off_dir;
    p.alpha = at->alpha; p.gamma = at->gamma; p.sigma = at->sigma;
    for (int j = 0; j < 7; ++j) p.cw[j] = at->code_weights[j];
    p.cls_weight = at->cls_weight; p.loc_weight = at->loc_weight; p.dir_weight = at->dir_weight;
    p.pos_cls_weight = at->pos_cls_weight; p.neg_cls_weight = at->neg_cls_weight;
    double *part = (double *)ws.ptr;
    int *counts = (int *)((char *)ws.ptr + w.counts);
    const uint16_t *head = (const uint16_t *)params[0];
    const int *labels = (const int *)params[1];
    const float *reg = (const float *)params[2], *anchors = (const float *)params[3];
    float *grad = with_grad ? (float *)params[7] : nullptr;
    const int vec = strip_vec(HW * C, head, grad);   // (a sample's H W C elements: C itself need not be a multiple of 8)
    const size_t lds = strip_lds_bytes(PPL_LDS_HEAD, PPL_STRIP, C, with_grad, A * 4);   // 8 A <= C <= 128: at most 176 + 64 (64 + 768) = 53424 bytes
    hipLaunchKernelGGL(pp_loss_count_kernel, dim3((unsigned)cps, (unsigned)B), dim3(256), 0, s, labels, (int)N, (int)cps, counts);
    grad_or_not(with_grad, [&](auto g) {
        hipLaunchKernelGGL(pp_loss_dense_kernel<decltype(g)::value>, dim3((unsigned)n_strips), dim3(256), lds, s, head, labels, reg, anchors, p, vec,
                           counts, part, grad);
    });
    hipLaunchKernelGGL(pp_loss_finish_kernel, dim3(1), dim3(256), 0, s, part, counts, p, (int)n_strips, (float *)params[4], (float *)params[5],
                       (float *)params[6]);
    return launched();
}

}  // namespace md

using namespace md;

extern "C" int64_t md_pp_loss_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t num_anchors) {
    return any_negative({B, H, W, num_anchors}) ? -1 : ws_answer(pp_loss_scratch(B, H, W, num_anchors).total);
}
extern "C" int md_pp_loss(MD_AOT_ARGS) { return pp_loss_entry(nparam, params, ndims, shapes, dtypes, stream, extra, false); }
extern "C" int md_pp_loss_grad(MD_AOT_ARGS) { return pp_loss_entry(nparam, params, ndims, shapes, dtypes, stream, extra, true); }
