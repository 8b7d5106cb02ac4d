// cocoeval.hip -- the COCO bbox AP evaluation on the device (include/minddet_hip_cocoeval.h): from a detector's (dets, count) and packed
// ground truth to the precision / recall tables of COCOeval.  minddet_amd/coco_eval.py states the same rules on the host and judges these.
//
//   md_coco_eval_rows        ce_rows_kernel    one workgroup per image: to_float of every taken row, the category counts, and each row's
//                                              place by counting the rows ahead of it under (k, -score, source row); keys in LDS
//   md_coco_eval_match       ce_fill_kernel    dtm = -1, dt_ig = 0 everywhere (rows outside every cell keep that)
//                            ce_match_kernel   one wave per (cell, area range): ground truths over the lanes in chunks of 64 (<= 4 per
//                                              lane, in registers), the matched set one bit per (threshold, chunk) in a 64-bit mask; per
//                                              detection the IoUs once, then per threshold one wave reduction on (counted before
//                                              ignored, IoU, row)
//   md_coco_eval_accumulate  ce_ngt_kernel     one workgroup per (area range, category): the integer sum of cell_ngt over the images
//                            ce_accum_kernel   one workgroup per (k, a, m, t): integer scans of tp / fp over the category's list in tiles
//                                              of 256, the maximum of pr per recall bucket in LDS (buckets rise with the list, so the
//                                              first lane of a run owns its bucket: no atomics), then a suffix maximum over the buckets
// Float64 without contraction, no floating-point atomics, no memset, no scratch: every buffer is an operand.  A cell whose rows leave the
// operands is skipped, per-cell counts are clamped to the limits: nothing is read or written out of bounds.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#include "aot.h"
#include "../../include/minddet_hip_cocoeval.h"
#include "workgroup.h"

namespace md {

static_assert(sizeof(md_coco_eval_rows_attrs) == 4, "minddet_hip_cocoeval.h: attribute struct layout");

constexpr const char *CE_F64 = "float64";
constexpr int CE_MAX_D = MD_COCOEVAL_MAX_DETS, CE_MAX_G = MD_COCOEVAL_MAX_GTS, CE_MAX_ROWS_IMG = MD_COCOEVAL_MAX_IMAGE_DETS;
constexpr int CE_MAX_K = MD_COCOEVAL_MAX_CATS, CE_MAX_T = MD_COCOEVAL_MAX_THRS, CE_MAX_R = MD_COCOEVAL_MAX_RECS;
constexpr int CE_CHUNKS = CE_MAX_G / 64;        // ground truths per lane
static_assert(CE_CHUNKS == 4 && CE_MAX_G % 64 == 0 && CE_MAX_T * CE_CHUNKS <= 64, "the matched set is one bit per (threshold, chunk) of a 64-bit mask");
static_assert(CE_MAX_R <= 256 && CE_MAX_K <= 256, "one lane per recall bucket / category in a workgroup of 256");

// numpy's minimum / maximum of two values: a NaN stays
__device__ __forceinline__ double ce_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double ce_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// float("{:.2f}".format(v)), exactly: p + e is v 100 without error, so a tie of p is a tie of the decimal string only when e == 0
__device__ __forceinline__ double ce_to_float(double v) {
    const double p = v * 100.0;
    const double e = fma(v, 100.0, -p);
    double n = rint(p);
    const double f = p - n;
    if (f == 0.5 && e > 0) n += 1.0;
    if (f == -0.5 && e < 0) n -= 1.0;
    return n / 100.0;
}

// ---------------------------------------------------------------------------------------------------- rows
struct RowsArgs {
    const float *dets; const int *count, *label_to_k;
    double *dt_box, *dt_area, *dt_score; int *dt_cat, *dt_rank, *dt_beg, *dt_cnt, *dt_src;
    int max_det, L, Kc, first;
};

__global__ __launch_bounds__(256) void ce_rows_kernel(RowsArgs a) {
    __shared__ int s_k[CE_MAX_ROWS_IMG];
    __shared__ double s_sc[CE_MAX_ROWS_IMG];
    __shared__ int s_beg[CE_MAX_K + 1], s_cnt[CE_MAX_K];
    const int tid = threadIdx.x, b = blockIdx.x, img = a.first + b;
    int n = a.count[b];
    n = n < 0 ? 0 : (n > a.max_det ? a.max_det : n);
    const float *d = a.dets + (int64_t)b * a.max_det * 6;
    for (int r = tid; r < a.max_det; r += 256) {
        int k = -1;
        double s = 0.0;
        if (r < n) {
            const float lab = d[r * 6 + 5];
            if (lab > -1.0f && lab < (float)a.L) {             // int(label) lies in [0, L); a NaN fails both
                const int kv = a.label_to_k[(int)lab];
                if (kv >= 0 && kv < a.Kc) { k = kv; s = ce_to_float((double)d[r * 6 + 4]); }
            }
        }
        s_k[r] = k;
        s_sc[r] = s;
    }
    __syncthreads();
    for (int k = tid; k < a.Kc; k += 256) {
        int c = 0;
        for (int r = 0; r < n; ++r) c += s_k[r] == k;
        s_cnt[k] = c < CE_MAX_D ? c : CE_MAX_D;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int k = 0; k < a.Kc; ++k) { s_beg[k] = acc; acc += s_cnt[k]; }
        s_beg[a.Kc] = acc;
    }
    __syncthreads();
    const int64_t row0 = (int64_t)img * a.max_det;
    for (int k = tid; k < a.Kc; k += 256) {
        a.dt_beg[(int64_t)img * a.Kc + k] = (int)(row0 + s_beg[k]);
        a.dt_cnt[(int64_t)img * a.Kc + k] = s_cnt[k];
    }
    for (int p = s_beg[a.Kc] + tid; p < a.max_det; p += 256) {     // the unused tail of the image's block
        const int64_t at = row0 + p;
        a.dt_box[at * 4] = 0.0; a.dt_box[at * 4 + 1] = 0.0; a.dt_box[at * 4 + 2] = 0.0; a.dt_box[at * 4 + 3] = 0.0;
        a.dt_area[at] = 0.0; a.dt_score[at] = 0.0;
        a.dt_cat[at] = a.Kc; a.dt_rank[at] = 0; a.dt_src[at] = -1;
    }
    for (int r = tid; r < n; r += 256) {
        const int k = s_k[r];
        if (k < 0) continue;
        const double s = s_sc[r];
        int rank = 0;                                         // the rows of the cell ahead of r: a higher score, or an equal one from an earlier row
        for (int q = 0; q < n; ++q)
            if (s_k[q] == k) rank += (s_sc[q] > s) || (s_sc[q] == s && q < r);
        if (rank >= CE_MAX_D) continue;
        const int64_t at = row0 + s_beg[k] + rank;
        const double x1 = (double)d[r * 6], y1 = (double)d[r * 6 + 1], x2 = (double)d[r * 6 + 2], y2 = (double)d[r * 6 + 3];
        const double w = ce_to_float(x2 - x1), h = ce_to_float(y2 - y1);
        a.dt_box[at * 4] = ce_to_float(x1); a.dt_box[at * 4 + 1] = ce_to_float(y1); a.dt_box[at * 4 + 2] = w; a.dt_box[at * 4 + 3] = h;
        a.dt_area[at] = w * h; a.dt_score[at] = s;
        a.dt_cat[at] = k; a.dt_rank[at] = rank; a.dt_src[at] = r;
    }
}

// ---------------------------------------------------------------------------------------------------- matching
struct MatchArgs {
    const int *gt_beg, *gt_cnt, *dt_beg, *dt_cnt;
    const double *gt_box, *gt_area; const uint8_t *gt_crowd, *gt_ignore; const double *dt_box, *dt_area, *iou_thr, *area_rng;
    int *dtm; uint8_t *dt_ig; int *cell_ngt;
    int64_t Gt, Dt;
    int C, T, A;
};

__global__ __launch_bounds__(256) void ce_fill_kernel(int *dtm, uint8_t *dt_ig, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) { dtm[i] = -1; dt_ig[i] = 0; }
}

__global__ __launch_bounds__(64) void ce_match_kernel(MatchArgs a) {
    const int lane = threadIdx.x, cell = blockIdx.x / a.A, ar = blockIdx.x % a.A;
    const double lo = a.area_rng[ar * 2], hi = a.area_rng[ar * 2 + 1];
    const int64_t g0 = a.gt_beg[cell], gc = a.gt_cnt[cell], d0 = a.dt_beg[cell], dc = a.dt_cnt[cell];
    const bool gok = g0 >= 0 && gc >= 0 && g0 + gc <= a.Gt, dok = d0 >= 0 && dc >= 0 && d0 + dc <= a.Dt;
    const int G = gok ? (int)(gc < CE_MAX_G ? gc : CE_MAX_G) : 0, D = dok ? (int)(dc < CE_MAX_D ? dc : CE_MAX_D) : 0;
    double gx1[CE_CHUNKS], gy1[CE_CHUNKS], gx2[CE_CHUNKS], gy2[CE_CHUNKS], ga[CE_CHUNKS];
    unsigned have = 0, crowd = 0, ign = 0;                    // one bit per chunk
    int counted = 0;
#pragma unroll
    for (int ch = 0; ch < CE_CHUNKS; ++ch) {
        const int g = lane + 64 * ch;
        gx1[ch] = gy1[ch] = gx2[ch] = gy2[ch] = ga[ch] = 0.0;
        if (g < G) {
            const int64_t row = g0 + g;
            const double *b = a.gt_box + row * 4;
            gx1[ch] = b[0]; gy1[ch] = b[1]; gx2[ch] = b[0] + b[2]; gy2[ch] = b[1] + b[3]; ga[ch] = b[2] * b[3];
            const double area = a.gt_area[row];
            const bool ig = a.gt_ignore[row] != 0 || area < lo || area > hi;
            have |= 1u << ch;
            crowd |= (unsigned)(a.gt_crowd[row] != 0) << ch;
            ign |= (unsigned)ig << ch;
            counted += !ig;
        }
    }
    counted = wave_sum_all(counted);
    if (lane == 0) a.cell_ngt[(int64_t)ar * a.C + cell] = counted;
    if (D == 0) return;
    if (G == 0) {                                             // nothing to match: the detections over the lanes
        for (int d = lane; d < D; d += 64) {
            const double darea = a.dt_area[d0 + d];
            const uint8_t out_rng = darea < lo || darea > hi;
            for (int t = 0; t < a.T; ++t) {
                const int64_t at = ((int64_t)ar * a.T + t) * a.Dt + d0 + d;
                a.dtm[at] = -1;
                a.dt_ig[at] = out_rng;
            }
        }
        return;
    }
    unsigned long long matched = 0;                           // bit t CE_CHUNKS + ch: a detection holds the lane's ground truth of chunk ch at threshold t
    for (int d = 0; d < D; ++d) {
        const int64_t row = d0 + d;
        const double *b = a.dt_box + row * 4;
        const double dx1 = b[0], dy1 = b[1], dx2 = b[0] + b[2], dy2 = b[1] + b[3], da = b[2] * b[3];
        const double darea = a.dt_area[row];
        const bool out_rng = darea < lo || darea > hi;
        double iou[CE_CHUNKS];
#pragma unroll
        for (int ch = 0; ch < CE_CHUNKS; ++ch) {
            double iw = ce_min(dx2, gx2[ch]) - ce_max(dx1, gx1[ch]);
            double ih = ce_min(dy2, gy2[ch]) - ce_max(dy1, gy1[ch]);
            iw = iw < 0 ? 0.0 : iw;
            ih = ih < 0 ? 0.0 : ih;
            const double inter = iw * ih;
            const double uni = (crowd >> ch & 1) ? da : (da + ga[ch]) - inter;
            iou[ch] = uni > 0 ? inter / uni : 0.0;
        }
        for (int t = 0; t < a.T; ++t) {
            const double thr = a.iou_thr[t], cap = 1 - 1e-10;
            const double bar = cap < thr ? cap : thr;         // min(t, 1 - 1e-10)
            const unsigned held = (unsigned)(matched >> (t * CE_CHUNKS)) & ((1u << CE_CHUNKS) - 1u);
            int bc = 0, bi = -1;                              // class of the best candidate: 2 counted, 1 ignored, 0 none
            double bo = 0.0;
#pragma unroll
            for (int ch = 0; ch < CE_CHUNKS; ++ch) {
                if ((have >> ch & 1) && (!(held >> ch & 1) || (crowd >> ch & 1)) && iou[ch] >= bar) {
                    const int cls = (ign >> ch & 1) ? 1 : 2;
                    if (cls > bc || (cls == bc && iou[ch] >= bo)) { bc = cls; bo = iou[ch]; bi = lane + 64 * ch; }      // the highest row on equal IoU
                }
            }
            for (int off = 32; off > 0; off >>= 1) {          // every lane ends with the winner
                const double oo = __shfl_xor(bo, off, 64);
                const int oc = __shfl_xor(bc, off, 64), oi = __shfl_xor(bi, off, 64);
                if (oc > bc || (oc == bc && oc > 0 && (oo > bo || (oo == bo && oi > bi)))) { bc = oc; bo = oo; bi = oi; }
            }
            if (bc > 0 && (bi & 63) == lane) matched |= 1ull << (t * CE_CHUNKS + (bi >> 6));
            if (lane == 0) {
                const int64_t at = ((int64_t)ar * a.T + t) * a.Dt + row;
                a.dtm[at] = bc > 0 ? (int)(g0 + bi) : -1;
                a.dt_ig[at] = bc > 0 ? (uint8_t)(bc == 1) : (uint8_t)out_rng;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- accumulate
struct AccumArgs {
    const int *order, *cat_off, *dt_rank, *dtm; const uint8_t *dt_ig; const int *cell_ngt; const double *rec_thr; const int *max_dets;
    double *precision, *recall; int *n_gt;
    int64_t Dt;
    int C, Kc, T, A, R, M;
};

__global__ __launch_bounds__(256) void ce_ngt_kernel(AccumArgs a) {
    __shared__ int red[4];
    const int ar = blockIdx.x / a.Kc, k = blockIdx.x % a.Kc, I = a.C / a.Kc;
    int n = 0;
    for (int i = threadIdx.x; i < I; i += 256) n += a.cell_ngt[(int64_t)ar * a.C + (int64_t)i * a.Kc + k];
    n = block_count(n, red);
    if (threadIdx.x == 0) a.n_gt[blockIdx.x] = n;
}

__global__ __launch_bounds__(256) void ce_accum_kernel(AccumArgs a) {
    __shared__ double s_thr[CE_MAX_R], s_q[CE_MAX_R], s_pr[256];
    __shared__ int s_b[256], wsum[4];
    const int tid = threadIdx.x;
    int id = blockIdx.x;
    const int t = id % a.T; id /= a.T;
    const int m = id % a.M; id /= a.M;
    const int ar = id % a.A, k = id / a.A;
    for (int r = tid; r < CE_MAX_R; r += 256) { s_thr[r] = r < a.R ? a.rec_thr[r] : 0.0; s_q[r] = 0.0; }
    const int ngt = a.n_gt[ar * a.Kc + k], md = a.max_dets[m];
    int64_t beg = a.cat_off[k], end = a.cat_off[k + 1];
    if (beg < 0 || end > a.Dt || end < beg) beg = end = 0;    // a list that leaves the operand is skipped
    const double eps = 2.220446049250313e-16;                 // np.spacing(1)
    int ctp = 0, cfp = 0;
    __syncthreads();
    if (ngt > 0) {
        for (int64_t base = beg; base < end; base += 256) {
            const int64_t j = base + tid;
            bool keep = false;
            int tpf = 0, fpf = 0;
            if (j < end) {
                const int64_t row = a.order[j];
                if (row >= 0 && row < a.Dt && a.dt_rank[row] < md) {
                    const int64_t at = ((int64_t)ar * a.T + t) * a.Dt + row;
                    const bool mt = a.dtm[at] >= 0, ig = a.dt_ig[at] != 0;
                    keep = true;
                    tpf = mt && !ig;
                    fpf = !mt && !ig;
                }
            }
            int all_tp, all_fp;
            const int tp = ctp + block_exclusive_scan<4>(tpf, wsum, all_tp) + tpf;
            const int fp = cfp + block_exclusive_scan<4>(fpf, wsum, all_fp) + fpf;
            const double rc = (double)tp / (double)ngt;
            const double pr = keep ? (double)tp / (((double)fp + (double)tp) + eps) : 0.0;
            int lo = 0, hi = a.R;                             // the number of recall thresholds <= rc
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_thr[mid] <= rc) lo = mid + 1; else hi = mid;
            }
            __syncthreads();                                  // the last tile's readers are done
            s_b[tid] = lo;
            s_pr[tid] = pr;
            __syncthreads();
            const int n_in = (int)(end - base < 256 ? end - base : 256);
            if (tid < n_in && lo > 0 && (tid == 0 || s_b[tid - 1] != lo)) {      // the first lane of a run of one bucket owns it
                double mx = pr;
                for (int e = tid + 1; e < n_in && s_b[e] == lo; ++e) mx = s_pr[e] > mx ? s_pr[e] : mx;
                if (mx > s_q[lo - 1]) s_q[lo - 1] = mx;
            }
            ctp += all_tp;
            cfp += all_fp;
        }
    }
    __syncthreads();
    if (tid < a.R) {
        double q = 0.0;                                       // the envelope: the maximum to the right
        for (int r = tid; r < a.R; ++r) q = s_q[r] > q ? s_q[r] : q;
        a.precision[((((int64_t)t * a.R + tid) * a.Kc + k) * a.A + ar) * a.M + m] = ngt > 0 ? q : -1.0;
    }
    if (tid == 0) a.recall[(((int64_t)t * a.Kc + k) * a.A + ar) * a.M + m] = ngt > 0 ? (double)ctp / (double)ngt : -1.0;
}

// the limits every op holds its extents to
static bool ce_too_large(int64_t C, int64_t Kc, int64_t Gt, int64_t Dt, int64_t T, int64_t A, int64_t R, int64_t M) {
    return C >= MD_COCOEVAL_MAX_CELLS || Kc > MD_COCOEVAL_MAX_CATS || Gt > MD_COCOEVAL_MAX_ROWS || Dt > MD_COCOEVAL_MAX_ROWS ||
           T > MD_COCOEVAL_MAX_THRS || A > MD_COCOEVAL_MAX_AREAS || R > MD_COCOEVAL_MAX_RECS || M > MD_COCOEVAL_MAX_MAXDETS ||
           mul({A, T, Dt}) >= ((int64_t)1 << 31);
}

}  // namespace md

using namespace md;

extern "C" int md_coco_eval_rows(MD_AOT_ARGS) {
    // in : dets[B,max_det,6] f32, count[B] i32, label_to_k[L] i32
    // out: dt_box[Dt,4] f64, dt_area[Dt] f64, dt_score[Dt] f64, dt_cat[Dt] i32, dt_rank[Dt] i32, dt_beg[C] i32, dt_cnt[C] i32, dt_src[Dt] i32
    Args a(MD_ARGS, 11, 11);
    const md_coco_eval_rows_attrs *at = a.attrs<md_coco_eval_rows_attrs>(extra);
    a.tensor(0, F32, 3); a.tensor(1, I32, 1); a.tensor(2, I32, 1); a.tensor(3, CE_F64, 2); a.tensor(4, CE_F64, 1); a.tensor(5, CE_F64, 1);
    a.tensor(6, I32, 1); a.tensor(7, I32, 1); a.tensor(8, I32, 1); a.tensor(9, I32, 1); a.tensor(10, I32, 1);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), max_det = a.d(0, 1), L = a.d(2, 0), Dt = a.d(3, 0), C = a.d(8, 0);
    a.require(B >= 0 && max_det >= 1 && a.d(0, 2) == 6 && a.d(1, 0) == B && L >= 1 && Dt >= 1 && C >= 1 && a.d(3, 1) == 4);
    a.require(a.d(4, 0) == Dt && a.d(5, 0) == Dt && a.d(6, 0) == Dt && a.d(7, 0) == Dt && a.d(9, 0) == C && a.d(10, 0) == Dt);
    if (int rc = a.rc()) return rc;
    a.require(Dt % max_det == 0 && C % (Dt / max_det) == 0);
    if (int rc = a.rc()) return rc;
    const int64_t I = Dt / max_det, Kc = C / I;
    a.require(at->first_image >= 0 && (int64_t)at->first_image + B <= I);
    if (int rc = a.rc()) return rc;
    if (max_det > MD_COCOEVAL_MAX_IMAGE_DETS || L > MD_COCOEVAL_MAX_LABELS || ce_too_large(C, Kc, 0, Dt, 0, 0, 0, 0)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10})) return MD_ERR_ARG;
    if (aliased(params, 3, 11)) return MD_ERR_ARG;
    if (B == 0) return MD_OK;
    RowsArgs k;
    k.dets = (const float *)params[0]; k.count = (const int *)params[1]; k.label_to_k = (const int *)params[2];
    k.dt_box = (double *)params[3]; k.dt_area = (double *)params[4]; k.dt_score = (double *)params[5]; k.dt_cat = (int *)params[6];
    k.dt_rank = (int *)params[7]; k.dt_beg = (int *)params[8]; k.dt_cnt = (int *)params[9]; k.dt_src = (int *)params[10];
    k.max_det = (int)max_det; k.L = (int)L; k.Kc = (int)Kc; k.first = at->first_image;
    hipLaunchKernelGGL(ce_rows_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, k);
    return launched();
}

extern "C" int md_coco_eval_match(MD_AOT_ARGS) {
    // in : gt_beg[C], gt_cnt[C], dt_beg[C], dt_cnt[C] i32, gt_box[Gt,4] f64, gt_area[Gt] f64, gt_crowd[Gt] u8, gt_ignore[Gt] u8, dt_box[Dt,4] f64,
    //      dt_area[Dt] f64, iou_thr[T] f64, area_rng[A,2] f64 ; out: dtm[A,T,Dt] i32, dt_ig[A,T,Dt] u8, cell_ngt[A,C] i32
    Args a(MD_ARGS, 15, 15);
    a.tensor(0, I32, 1); a.tensor(1, I32, 1); a.tensor(2, I32, 1); a.tensor(3, I32, 1); a.tensor(4, CE_F64, 2); a.tensor(5, CE_F64, 1);
    a.tensor(6, U8, 1); a.tensor(7, U8, 1); a.tensor(8, CE_F64, 2); a.tensor(9, CE_F64, 1); a.tensor(10, CE_F64, 1); a.tensor(11, CE_F64, 2);
    a.tensor(12, I32, 3); a.tensor(13, U8, 3); a.tensor(14, I32, 2);
    if (int rc = a.rc()) return rc;
    const int64_t C = a.d(0, 0), Gt = a.d(4, 0), Dt = a.d(8, 0), T = a.d(10, 0), A = a.d(11, 0);
    a.require(C >= 1 && Gt >= 0 && Dt >= 0 && T >= 1 && A >= 1 && a.d(1, 0) == C && a.d(2, 0) == C && a.d(3, 0) == C && a.d(4, 1) == 4);
    a.require(a.d(5, 0) == Gt && a.d(6, 0) == Gt && a.d(7, 0) == Gt && a.d(8, 1) == 4 && a.d(9, 0) == Dt && a.d(11, 1) == 2);
    a.require(a.d(12, 0) == A && a.d(12, 1) == T && a.d(12, 2) == Dt && a.d(13, 0) == A && a.d(13, 1) == T && a.d(13, 2) == Dt && a.d(14, 0) == A &&
              a.d(14, 1) == C);
    if (int rc = a.rc()) return rc;
    if (ce_too_large(C, 0, Gt, Dt, T, A, 0, 0)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14})) return MD_ERR_ARG;
    if (aliased(params, 12, 15)) return MD_ERR_ARG;
    MatchArgs k;
    k.gt_beg = (const int *)params[0]; k.gt_cnt = (const int *)params[1]; k.dt_beg = (const int *)params[2]; k.dt_cnt = (const int *)params[3];
    k.gt_box = (const double *)params[4]; k.gt_area = (const double *)params[5]; k.gt_crowd = (const uint8_t *)params[6];
    k.gt_ignore = (const uint8_t *)params[7]; k.dt_box = (const double *)params[8]; k.dt_area = (const double *)params[9];
    k.iou_thr = (const double *)params[10]; k.area_rng = (const double *)params[11];
    k.dtm = (int *)params[12]; k.dt_ig = (uint8_t *)params[13]; k.cell_ngt = (int *)params[14];
    k.Gt = Gt; k.Dt = Dt; k.C = (int)C; k.T = (int)T; k.A = (int)A;
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = A * T * Dt;
    if (total > 0) hipLaunchKernelGGL(ce_fill_kernel, dim3(grid1d((size_t)total)), dim3(256), 0, s, k.dtm, k.dt_ig, total);
    hipLaunchKernelGGL(ce_match_kernel, dim3((unsigned)(C * A)), dim3(64), 0, s, k);
    return launched();
}

extern "C" int md_coco_eval_accumulate(MD_AOT_ARGS) {
    // in : order[Dt] i32, cat_off[Kc+1] i32, dt_rank[Dt] i32, dtm[A,T,Dt] i32, dt_ig[A,T,Dt] u8, cell_ngt[A,C] i32, rec_thr[R] f64, max_dets[M] i32
    // out: precision[T,R,Kc,A,M] f64, recall[T,Kc,A,M] f64, n_gt[A,Kc] i32
    Args a(MD_ARGS, 11, 11);
    a.tensor(0, I32, 1); a.tensor(1, I32, 1); a.tensor(2, I32, 1); a.tensor(3, I32, 3); a.tensor(4, U8, 3); a.tensor(5, I32, 2);
    a.tensor(6, CE_F64, 1); a.tensor(7, I32, 1); a.tensor(8, CE_F64, 5); a.tensor(9, CE_F64, 4); a.tensor(10, I32, 2);
    if (int rc = a.rc()) return rc;
    const int64_t Dt = a.d(0, 0), Kc = a.d(1, 0) - 1, A = a.d(3, 0), T = a.d(3, 1), C = a.d(5, 1), R = a.d(6, 0), M = a.d(7, 0);
    a.require(Dt >= 0 && Kc >= 1 && A >= 1 && T >= 1 && C >= 1 && R >= 1 && M >= 1 && a.d(2, 0) == Dt && a.d(3, 2) == Dt && a.d(4, 0) == A &&
              a.d(4, 1) == T && a.d(4, 2) == Dt && a.d(5, 0) == A);
    a.require(a.d(8, 0) == T && a.d(8, 1) == R && a.d(8, 2) == Kc && a.d(8, 3) == A && a.d(8, 4) == M && a.d(9, 0) == T && a.d(9, 1) == Kc &&
              a.d(9, 2) == A && a.d(9, 3) == M && a.d(10, 0) == A && a.d(10, 1) == Kc);
    if (int rc = a.rc()) return rc;
    a.require(C % Kc == 0);
    if (int rc = a.rc()) return rc;
    if (ce_too_large(C, Kc, 0, Dt, T, A, R, M)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10})) return MD_ERR_ARG;
    if (aliased(params, 8, 11)) return MD_ERR_ARG;
    AccumArgs k;
    k.order = (const int *)params[0]; k.cat_off = (const int *)params[1]; k.dt_rank = (const int *)params[2]; k.dtm = (const int *)params[3];
    k.dt_ig = (const uint8_t *)params[4]; k.cell_ngt = (const int *)params[5]; k.rec_thr = (const double *)params[6];
    k.max_dets = (const int *)params[7]; k.precision = (double *)params[8]; k.recall = (double *)params[9]; k.n_gt = (int *)params[10];
    k.Dt = Dt; k.C = (int)C; k.Kc = (int)Kc; k.T = (int)T; k.A = (int)A; k.R = (int)R; k.M = (int)M;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ce_ngt_kernel, dim3((unsigned)(A * Kc)), dim3(256), 0, s, k);
    hipLaunchKernelGGL(ce_accum_kernel, dim3((unsigned)(Kc * A * M * T)), dim3(256), 0, s, k);
    return launched();
}
