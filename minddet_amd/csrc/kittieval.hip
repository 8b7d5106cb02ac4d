// kittieval.hip -- the KITTI AP evaluation on the device (include/minddet_hip_kittieval.h): from packed annotations to the
// [class, difficulty, overlap level, 41] count tables.  minddet_amd/kitti_eval.py states the same rules on the host and judges these.
//
//   md_kitti_eval_flags       ke_flags_kernel       one lane per (class, difficulty, row): clean_data's flags as 1 + flag
//                             ke_valid_kernel       one workgroup per (class, difficulty): the counted ground truths (block_count)
//   md_kitti_eval_overlaps    ke_overlaps_kernel    one lane per pair, its image by a binary search of ov_off (<= 17 steps); the rotated
//                                                   pairs through rot_eval.h's rie_pair, polygon scratch in LDS as md_rotate_iou_eval's
//   md_kitti_eval_match       ke_match_kernel       one wave per (image, task): detections over the lanes in chunks of 64 (<= 8 per lane,
//                                                   in registers), the assigned set a per-lane bit mask; per ground truth one contiguous
//                                                   read of its overlap row and one wave reduction on (score, index)
//   md_kitti_eval_thresholds  ke_thresholds_kernel  one lane per task: the recurrence of get_thresholds
//   md_kitti_eval_stats       ke_stats_kernel       the wave of ke_match_kernel looping over the task's thresholds, reduction on
//                                                   (counted before ignored, overlap, index); ke_sum_kernel: one workgroup per
//                                                   (task, threshold), integer block sums and the float64 sum in image order
// Float64 without contraction, no floating-point atomics, no memset, no scratch: every buffer is an operand.  An image whose offsets
// leave the operands is skipped, per-image extents are clamped to the limits: nothing is read or written out of bounds.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#include "aot.h"
#include "../../include/minddet_hip_kittieval.h"
#include "rot_eval.h"
#include "workgroup.h"

namespace md {

static_assert(sizeof(md_kitti_eval_flags_attrs) == 4 && sizeof(md_kitti_eval_overlaps_attrs) == 4 && sizeof(md_kitti_eval_stats_attrs) == 8,
              "minddet_hip_kittieval.h: attribute struct layout");

constexpr const char *KE_F64 = "float64";
constexpr int KE_MAX_D = MD_KEVAL_MAX_DETS, KE_MAX_G = MD_KEVAL_MAX_GTS, KE_PTS = MD_KEVAL_SAMPLE_PTS;
constexpr int KE_CHUNKS = KE_MAX_D / 64;        // detections per lane
static_assert(KE_CHUNKS == 8 && KE_MAX_D % 64 == 0, "the per-lane assigned mask and register arrays hold 8 detections");

// numpy's minimum / maximum of two values: a NaN stays
__device__ __forceinline__ double ke_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double ke_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// image_box_overlap (eval_gpu/eval.py:91-121) of one pair; criterion -1: IoU, 0: over the area of b
__device__ __forceinline__ double ke_image_overlap(const double *b, const double *q, int criterion) {
    const double iw = ke_min(b[2], q[2]) - ke_max(b[0], q[0]);
    const double ih = ke_min(b[3], q[3]) - ke_max(b[1], q[1]);
    if (!(iw > 0 && ih > 0)) return 0.0;
    const double inter = iw * ih;
    const double a = (b[2] - b[0]) * (b[3] - b[1]), qa = (q[2] - q[0]) * (q[3] - q[1]);
    const double ua = criterion == -1 ? (a + qa) - inter : a + 0 * qa;
    return inter / ua;
}

// ---------------------------------------------------------------------------------------------------- flags
struct FlagArgs {
    const double *gt_box; const int *gt_occ; const double *gt_trunc; const uint8_t *gt_valid; const double *dt_box; const uint8_t *dt_same;
    uint8_t *ign_gt, *ign_dt; int *num_valid;
    int64_t Gt, Dt;
    int Cn, abs_h;
};

__constant__ double ke_min_height[3] = {40, 25, 25};
__constant__ int ke_max_occ[3] = {0, 1, 2};
__constant__ double ke_max_trunc[3] = {0.15, 0.3, 0.5};

__global__ __launch_bounds__(256) void ke_flags_kernel(FlagArgs a) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t ng = (int64_t)a.Cn * 3 * a.Gt, nd = (int64_t)a.Cn * 3 * a.Dt;
    if (id < ng) {
        const int64_t r = id % a.Gt;
        const int cd = (int)(id / a.Gt), c = cd / 3, d = cd % 3;
        const double *b = a.gt_box + r * 4;
        double height = b[3] - b[1];
        if (a.abs_h) height = fabs(height);
        const int valid = (int)a.gt_valid[(int64_t)c * a.Gt + r] - 1;
        const bool ignore = a.gt_occ[r] > ke_max_occ[d] || a.gt_trunc[r] > ke_max_trunc[d] || height <= ke_min_height[d];
        int flag;
        if (valid == 1 && !ignore) flag = 0;
        else if (valid == 0 || (ignore && valid == 1)) flag = 1;
        else flag = -1;
        a.ign_gt[id] = (uint8_t)(1 + flag);
    } else if (id < ng + nd) {
        const int64_t e = id - ng, r = e % a.Dt;
        const int c = (int)(e / a.Dt) / 3, d = (int)(e / a.Dt) % 3;
        const double *b = a.dt_box + r * 4;
        const double height = fabs(b[3] - b[1]);
        int flag;
        if (height < ke_min_height[d]) flag = 1;
        else if (a.dt_same[(int64_t)c * a.Dt + r]) flag = 0;
        else flag = -1;
        a.ign_dt[e] = (uint8_t)(1 + flag);
    }
}

__global__ __launch_bounds__(256) void ke_valid_kernel(FlagArgs a) {
    __shared__ int red[4];
    const uint8_t *f = a.ign_gt + (int64_t)blockIdx.x * a.Gt;
    int n = 0;
    for (int64_t r = threadIdx.x; r < a.Gt; r += 256) n += f[r] == 1;
    n = block_count(n, red);
    if (threadIdx.x == 0) a.num_valid[blockIdx.x] = n;
}

// ---------------------------------------------------------------------------------------------------- overlaps
struct OverlapArgs {
    const int *gt_off, *dt_off; const int64_t *ov_off; const double *gt, *dt;
    double *ov;
    int64_t Gt, Dt, P;
    int I, metric;
};

__global__ __launch_bounds__(256) void ke_overlaps_kernel(OverlapArgs a) {
    __shared__ float scratch[RIE_LDS_FLOATS];
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.P) return;
    double v = 0.0;
    bool pair = a.I > 0 && idx >= a.ov_off[0] && idx < a.ov_off[a.I];
    int64_t gi = 0, di = 0;
    if (pair) {
        int lo = 0, hi = a.I;                               // the last image whose block starts at or before idx
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.ov_off[mid] <= idx) lo = mid; else hi = mid;
        }
        const int64_t local = idx - a.ov_off[lo];
        const int g0 = a.gt_off[lo], d0 = a.dt_off[lo], G = a.gt_off[lo + 1] - g0, D = a.dt_off[lo + 1] - d0;
        pair = G > 0 && D > 0 && g0 >= 0 && d0 >= 0 && local / D < G;
        if (pair) {
            gi = g0 + local / D;
            di = d0 + local % D;
            pair = gi < a.Gt && di < a.Dt;
        }
    }
    if (pair) {
        if (a.metric == 0) {
            v = ke_image_overlap(a.dt + di * 4, a.gt + gi * 4, -1);
        } else {
            const double *b = a.dt + di * 7, *q = a.gt + gi * 7;      // (x, y, z, l, h, w, ry): the detection is the box, the ground truth the query
            const float r1[5] = {(float)b[0], (float)b[2], (float)b[3], (float)b[5], (float)b[6]};
            const float r2[5] = {(float)q[0], (float)q[2], (float)q[3], (float)q[5], (float)q[6]};
            if (a.metric == 1) {
                v = (double)rie_pair(r1, r2, -1, scratch);
            } else {
                const double rinc = (double)rie_pair(r1, r2, 2, scratch);
                const double ih = ke_min(b[1], q[1]) - ke_max(b[1] - b[4], q[1] - q[4]);
                const double v1 = b[3] * b[4] * b[5], v2 = q[3] * q[4] * q[5];
                const double inc = ih * rinc;
                const double out = (rinc > 0 && ih > 0) ? inc / ((v1 + v2) - inc) : 0.0;
                v = rinc > 0 ? out : rinc;
            }
        }
    }
    a.ov[idx] = v;
}

// ---------------------------------------------------------------------------------------------------- matching
struct MatchArgs {
    const double *ov; const uint8_t *ign_gt, *ign_dt; const double *score; const int *gt_off, *dt_off; const int64_t *ov_off;
    const double *min_ov, *thresholds; const int *nthresh;
    const double *gt_box; const uint8_t *gt_dc; const double *dt_box, *gt_alpha, *dt_alpha;
    double *matched;
    int *img_counts; double *img_sim; int *pr_counts; double *pr_sim;
    int64_t Gt, Dt, P;
    int I, Cn, K, metric, aos;
};

// the rows of image i: G, D clamped to the limits (stride: the block's true row length); an image whose offsets leave the operands has none
struct ImageRows { int g0, d0, G, D, stride; int64_t o0, G_all; };
__device__ __forceinline__ ImageRows image_rows(const MatchArgs &a, int i) {
    ImageRows r;
    r.g0 = a.gt_off[i]; r.d0 = a.dt_off[i]; r.o0 = a.ov_off[i];
    const int g1 = a.gt_off[i + 1], d1 = a.dt_off[i + 1];
    const int64_t G = (int64_t)g1 - r.g0, D = (int64_t)d1 - r.d0;
    const bool ok = r.g0 >= 0 && r.d0 >= 0 && G >= 0 && D >= 0 && g1 <= a.Gt && d1 <= a.Dt && r.o0 >= 0 && r.o0 + G * D <= a.P;
    r.stride = ok ? (int)D : 0;
    r.G_all = ok ? G : 0;
    r.G = ok ? (int)(G < KE_MAX_G ? G : KE_MAX_G) : 0;
    r.D = ok ? (int)(D < KE_MAX_D ? D : KE_MAX_D) : 0;
    return r;
}

// the lane's detections of the image: score and flag code (0 behind D: never a candidate)
__device__ __forceinline__ void load_dets(const MatchArgs &a, const ImageRows &r, int cd, double *sc, int *fl) {
    const int lane = threadIdx.x;
#pragma unroll
    for (int ch = 0; ch < KE_CHUNKS; ++ch) {
        const int d = lane + 64 * ch;
        sc[ch] = 0.0;
        fl[ch] = 0;
        if (d < r.D) {
            sc[ch] = a.score[r.d0 + d];
            fl[ch] = a.ign_dt[(int64_t)cd * a.Dt + r.d0 + d];
        }
    }
}

__global__ __launch_bounds__(64) void ke_match_kernel(MatchArgs a) {
    const int lane = threadIdx.x, T = a.Cn * 3 * a.K;
    const int task = blockIdx.x % T, i = blockIdx.x / T, cd = task / a.K, c = cd / 3, k = task % a.K;
    const ImageRows r = image_rows(a, i);
    const double mo = a.min_ov[c * a.K + k];
    double sc[KE_CHUNKS];
    int fl[KE_CHUNKS];
    load_dets(a, r, cd, sc, fl);
    const uint8_t *ig = a.ign_gt + (int64_t)cd * a.Gt + r.g0;
    double *out = a.matched + (int64_t)task * a.Gt + r.g0;
    unsigned assigned = 0;
    for (int g = 0; g < r.G; ++g) {
        const int fg = ig[g];
        double res = -INFINITY;
        if (fg != 0) {
            const double *row = a.ov + r.o0 + (int64_t)g * r.stride;
            double bs = 0.0;
            int bi = -1, bf = 0;
#pragma unroll
            for (int ch = 0; ch < KE_CHUNKS; ++ch) {
                const int d = lane + 64 * ch;
                if (d < r.D && fl[ch] != 0 && !(assigned >> ch & 1) && row[d] > mo && (bi < 0 || sc[ch] > bs)) { bs = sc[ch]; bi = d; bf = fl[ch]; }
            }
            for (int off = 32; off > 0; off >>= 1) {          // highest score, lowest index on equal scores; every lane ends with the winner
                const double os = __shfl_xor(bs, off, 64);
                const int oi = __shfl_xor(bi, off, 64), of = __shfl_xor(bf, off, 64);
                if (oi >= 0 && (bi < 0 || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; bf = of; }
            }
            if (bi >= 0) {
                if ((bi & 63) == lane) assigned |= 1u << (bi >> 6);
                if (fg == 1 && bf == 1) res = bs;
            }
        }
        if (lane == 0) out[g] = res;
    }
    for (int64_t g = r.G + lane; g < r.G_all; g += 64) out[g] = -INFINITY;      // rows beyond the limit: never matched
}

__global__ __launch_bounds__(64) void ke_thresholds_kernel(const double *sorted, const int *num_valid, double *thresholds, int *nthresh,
                                                           int T, int K, int64_t Gt) {
    const int task = blockIdx.x * 64 + threadIdx.x;
    if (task >= T) return;
    const double *s = sorted + (int64_t)task * Gt;
    double *out = thresholds + (int64_t)task * KE_PTS;
    const double num_gt = (double)num_valid[task / K];
    double current_recall = 0.0;
    int nt = 0;
    for (int64_t i = 0; i < Gt; ++i) {
        const double score = s[i];
        if (!(score > -INFINITY)) break;
        const bool last = i + 1 >= Gt || !(s[i + 1] > -INFINITY);
        const double l_recall = (double)(i + 1) / num_gt;
        const double r_recall = last ? l_recall : (double)(i + 2) / num_gt;
        if ((r_recall - current_recall) < (current_recall - l_recall) && !last) continue;
        if (nt < KE_PTS) out[nt] = score;
        ++nt;
        current_recall += 1 / 40.0;
    }
    nt = nt < KE_PTS ? nt : KE_PTS;
    for (int t = nt; t < KE_PTS; ++t) out[t] = NAN;
    nthresh[task] = nt;
}

__global__ __launch_bounds__(64) void ke_stats_kernel(MatchArgs a) {
    const int lane = threadIdx.x, T = a.Cn * 3 * a.K;
    const int task = blockIdx.x % T, i = blockIdx.x / T, cd = task / a.K, c = cd / 3, k = task % a.K;
    const ImageRows r = image_rows(a, i);
    const double mo = a.min_ov[c * a.K + k];
    double sc[KE_CHUNKS];
    int fl[KE_CHUNKS];
    load_dets(a, r, cd, sc, fl);
    unsigned in_dc = 0;                                       // the lane's detections inside a DontCare box of the image
    if (a.metric == 0) {
        for (int g = 0; g < r.G; ++g) {
            if (!a.gt_dc[r.g0 + g]) continue;
            const double *q = a.gt_box + (int64_t)(r.g0 + g) * 4;
#pragma unroll
            for (int ch = 0; ch < KE_CHUNKS; ++ch) {
                const int d = lane + 64 * ch;
                if (d < r.D && ke_image_overlap(a.dt_box + (int64_t)(r.d0 + d) * 4, q, 0) > mo) in_dc |= 1u << ch;
            }
        }
    }
    const uint8_t *ig = a.ign_gt + (int64_t)cd * a.Gt + r.g0;
    int nth = a.nthresh[task];
    nth = nth < 0 ? 0 : (nth > KE_PTS ? KE_PTS : nth);
    for (int t = 0; t < KE_PTS; ++t) {
        int tp = 0, fp = 0, fn = 0;
        double sim = 0.0;
        if (t < nth) {
            const double thresh = a.thresholds[(int64_t)task * KE_PTS + t];
            unsigned below = 0, assigned = 0;
#pragma unroll
            for (int ch = 0; ch < KE_CHUNKS; ++ch) below |= (unsigned)(sc[ch] < thresh) << ch;
            for (int g = 0; g < r.G; ++g) {
                const int fg = ig[g];
                if (fg == 0) continue;
                const double *row = a.ov + r.o0 + (int64_t)g * r.stride;
                int bc = 0, bi = -1;                          // class of the best candidate: 2 counted, 1 ignored, 0 none
                double bo = 0.0;
#pragma unroll
                for (int ch = 0; ch < KE_CHUNKS; ++ch) {
                    const int d = lane + 64 * ch;
                    if (d < r.D && fl[ch] != 0 && !((assigned | below) >> ch & 1)) {
                        const double o = row[d];
                        if (o > mo) {
                            const int cls = fl[ch] == 1 ? 2 : 1;
                            const double key = cls == 2 ? o : 0.0;      // among ignored candidates the first wins
                            if (cls > bc || (cls == bc && key > bo)) { bc = cls; bo = key; bi = d; }
                        }
                    }
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const double oo = __shfl_xor(bo, off, 64);
                    const int oc = __shfl_xor(bc, off, 64), oi = __shfl_xor(bi, off, 64);
                    if (oc > bc || (oc == bc && oc > 0 && (oo > bo || (oo == bo && oi < bi)))) { bc = oc; bo = oo; bi = oi; }
                }
                if (bc == 0) {
                    fn += fg == 1;
                } else {
                    if ((bi & 63) == lane) assigned |= 1u << (bi >> 6);
                    if (fg == 1 && bc == 2) {
                        ++tp;
                        if (a.aos) sim = sim + (1.0 + cos(a.gt_alpha[r.g0 + g] - a.dt_alpha[r.d0 + bi])) / 2.0;
                    }
                }
            }
            int n = 0;
#pragma unroll
            for (int ch = 0; ch < KE_CHUNKS; ++ch) n += fl[ch] == 1 && !((assigned | below | in_dc) >> ch & 1);
            fp = wave_sum_all(n);
        }
        if (lane == 0) {
            const int64_t at = ((int64_t)task * KE_PTS + t) * a.I + i;
            a.img_counts[at * 3] = tp; a.img_counts[at * 3 + 1] = fp; a.img_counts[at * 3 + 2] = fn;
            a.img_sim[at] = sim;
        }
    }
}

__global__ __launch_bounds__(256) void ke_sum_kernel(MatchArgs a) {
    __shared__ int red[4];
    __shared__ double buf[256];
    const int64_t base = (int64_t)blockIdx.x * a.I;           // blockIdx.x = task * 41 + threshold
    int n[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < a.I; i += 256)
        for (int e = 0; e < 3; ++e) n[e] += a.img_counts[(base + i) * 3 + e];
    for (int e = 0; e < 3; ++e) {
        const int v = block_count(n[e], red);
        if (threadIdx.x == 0) a.pr_counts[(int64_t)blockIdx.x * 3 + e] = v;
    }
    double s = 0.0;                                           // the images in order from 0, one term at a time
    for (int i0 = 0; i0 < a.I; i0 += 256) {
        const int i = i0 + threadIdx.x;
        __syncthreads();
        buf[threadIdx.x] = i < a.I ? a.img_sim[base + i] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = a.I - i0 < 256 ? a.I - i0 : 256;
            for (int e = 0; e < m; ++e) s = s + buf[e];
        }
    }
    if (threadIdx.x == 0) a.pr_sim[blockIdx.x] = s;
}

// the limits every op holds its extents to
static bool ke_too_large(int64_t I, int64_t Cn, int64_t K, int64_t Gt, int64_t Dt, int64_t P) {
    return I > MD_KEVAL_MAX_IMAGES || Cn > MD_KEVAL_MAX_CLASSES || K > MD_KEVAL_MAX_LEVELS || Gt > (int64_t)MD_KEVAL_MAX_IMAGES * KE_MAX_G ||
           Dt > (int64_t)MD_KEVAL_MAX_IMAGES * KE_MAX_D || P >= ((int64_t)1 << 31);
}

// operands 0 .. 7 of md_kitti_eval_match and md_kitti_eval_stats: ov[P], ign_gt[Cn,3,Gt], ign_dt[Cn,3,Dt], dt_score[Dt], gt_off[I+1],
// dt_off[I+1], ov_off[I+1], min_overlap[Cn,K]
static void match_operands(Args &a, int64_t &I, int64_t &Cn, int64_t &K, int64_t &Gt, int64_t &Dt, int64_t &P) {
    a.tensor(0, KE_F64, 1); a.tensor(1, U8, 3); a.tensor(2, U8, 3); a.tensor(3, KE_F64, 1); a.tensor(4, I32, 1); a.tensor(5, I32, 1);
    a.tensor(6, I64, 1); a.tensor(7, KE_F64, 2);
    P = a.d(0, 0); Cn = a.d(1, 0); Gt = a.d(1, 2); Dt = a.d(2, 2); I = a.d(4, 0) - 1; K = a.d(7, 1);
    a.require(P >= 0 && Cn >= 1 && Gt >= 0 && Dt >= 0 && I >= 0 && K >= 1 && a.d(1, 1) == 3 && a.d(2, 0) == Cn && a.d(2, 1) == 3);
    a.require(a.d(3, 0) == Dt && a.d(5, 0) == I + 1 && a.d(6, 0) == I + 1 && a.d(7, 0) == Cn);
}
static void match_pointers(MatchArgs &k, void **params, int64_t I, int64_t Cn, int64_t K, int64_t Gt, int64_t Dt, int64_t P) {
    k = MatchArgs{};
    k.ov = (const double *)params[0]; k.ign_gt = (const uint8_t *)params[1]; k.ign_dt = (const uint8_t *)params[2];
    k.score = (const double *)params[3]; k.gt_off = (const int *)params[4]; k.dt_off = (const int *)params[5];
    k.ov_off = (const int64_t *)params[6]; k.min_ov = (const double *)params[7];
    k.Gt = Gt; k.Dt = Dt; k.P = P; k.I = (int)I; k.Cn = (int)Cn; k.K = (int)K;
}

}  // namespace md

using namespace md;

extern "C" int md_kitti_eval_flags(MD_AOT_ARGS) {
    // in : gt_box[Gt,4] f64, gt_occ[Gt] i32, gt_trunc[Gt] f64, gt_valid[Cn,Gt] u8, dt_box[Dt,4] f64, dt_same[Cn,Dt] u8
    // out: ign_gt[Cn,3,Gt] u8, ign_dt[Cn,3,Dt] u8, num_valid[Cn,3] i32
    Args a(MD_ARGS, 9, 9);
    const md_kitti_eval_flags_attrs *at = a.attrs<md_kitti_eval_flags_attrs>(extra);
    a.tensor(0, KE_F64, 2); a.tensor(1, I32, 1); a.tensor(2, KE_F64, 1); a.tensor(3, U8, 2); a.tensor(4, KE_F64, 2); a.tensor(5, U8, 2);
    a.tensor(6, U8, 3); a.tensor(7, U8, 3); a.tensor(8, I32, 2);
    if (int rc = a.rc()) return rc;
    const int64_t Gt = a.d(0, 0), Dt = a.d(4, 0), Cn = a.d(3, 0);
    a.require(Gt >= 0 && Dt >= 0 && Cn >= 1 && a.d(0, 1) == 4 && a.d(1, 0) == Gt && a.d(2, 0) == Gt && a.d(3, 1) == Gt && a.d(4, 1) == 4);
    a.require(a.d(5, 0) == Cn && a.d(5, 1) == Dt && a.d(6, 0) == Cn && a.d(6, 1) == 3 && a.d(6, 2) == Gt && a.d(7, 0) == Cn && a.d(7, 1) == 3 &&
              a.d(7, 2) == Dt && a.d(8, 0) == Cn && a.d(8, 1) == 3);
    a.require(at->abs_gt_height == 0 || at->abs_gt_height == 1);
    if (int rc = a.rc()) return rc;
    if (ke_too_large(0, Cn, 0, Gt, Dt, 0)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8})) return MD_ERR_ARG;
    if (aliased(params, 6, 9)) return MD_ERR_ARG;
    FlagArgs k;
    k.gt_box = (const double *)params[0]; k.gt_occ = (const int *)params[1]; k.gt_trunc = (const double *)params[2];
    k.gt_valid = (const uint8_t *)params[3]; k.dt_box = (const double *)params[4]; k.dt_same = (const uint8_t *)params[5];
    k.ign_gt = (uint8_t *)params[6]; k.ign_dt = (uint8_t *)params[7]; k.num_valid = (int *)params[8];
    k.Gt = Gt; k.Dt = Dt; k.Cn = (int)Cn; k.abs_h = at->abs_gt_height;
    const int64_t total = Cn * 3 * (Gt + Dt);
    hipStream_t s = (hipStream_t)stream;
    if (total > 0) hipLaunchKernelGGL(ke_flags_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, k);
    hipLaunchKernelGGL(ke_valid_kernel, dim3((unsigned)(Cn * 3)), dim3(256), 0, s, k);
    return launched();
}

extern "C" int md_kitti_eval_overlaps(MD_AOT_ARGS) {
    // in : gt_off[I+1] i32, dt_off[I+1] i32, ov_off[I+1] i64, gt[Gt,W] f64, dt[Dt,W] f64 ; out: ov[P] f64
    Args a(MD_ARGS, 6, 6);
    const md_kitti_eval_overlaps_attrs *at = a.attrs<md_kitti_eval_overlaps_attrs>(extra);
    a.tensor(0, I32, 1); a.tensor(1, I32, 1); a.tensor(2, I64, 1); a.tensor(3, KE_F64, 2); a.tensor(4, KE_F64, 2); a.tensor(5, KE_F64, 1);
    if (int rc = a.rc()) return rc;
    const int64_t I = a.d(0, 0) - 1, Gt = a.d(3, 0), Dt = a.d(4, 0), P = a.d(5, 0);
    a.require(at->metric >= 0 && at->metric <= 2);
    if (int rc = a.rc()) return rc;
    const int64_t W = at->metric == 0 ? 4 : 7;
    a.require(I >= 0 && Gt >= 0 && Dt >= 0 && P >= 0 && a.d(1, 0) == I + 1 && a.d(2, 0) == I + 1 && a.d(3, 1) == W && a.d(4, 1) == W);
    if (int rc = a.rc()) return rc;
    if (ke_too_large(I, 0, 0, Gt, Dt, P)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5})) return MD_ERR_ARG;
    if (aliased(params, 5, 6)) return MD_ERR_ARG;
    if (P == 0) return MD_OK;
    OverlapArgs k;
    k.gt_off = (const int *)params[0]; k.dt_off = (const int *)params[1]; k.ov_off = (const int64_t *)params[2];
    k.gt = (const double *)params[3]; k.dt = (const double *)params[4]; k.ov = (double *)params[5];
    k.Gt = Gt; k.Dt = Dt; k.P = P; k.I = (int)I; k.metric = at->metric;
    hipLaunchKernelGGL(ke_overlaps_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k);
    return launched();
}

extern "C" int md_kitti_eval_match(MD_AOT_ARGS) {
    // in : the eight operands of match_operands ; out: matched[Cn,3,K,Gt] f64
    Args a(MD_ARGS, 9, 9);
    int64_t I, Cn, K, Gt, Dt, P;
    match_operands(a, I, Cn, K, Gt, Dt, P);
    a.tensor(8, KE_F64, 4);
    if (int rc = a.rc()) return rc;
    a.require(a.d(8, 0) == Cn && a.d(8, 1) == 3 && a.d(8, 2) == K && a.d(8, 3) == Gt);
    if (int rc = a.rc()) return rc;
    if (ke_too_large(I, Cn, K, Gt, Dt, P)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8})) return MD_ERR_ARG;
    if (aliased(params, 8, 9)) return MD_ERR_ARG;
    if (I == 0 || Gt == 0) return MD_OK;
    MatchArgs k;
    match_pointers(k, params, I, Cn, K, Gt, Dt, P);
    k.matched = (double *)params[8];
    hipLaunchKernelGGL(ke_match_kernel, dim3((unsigned)(I * Cn * 3 * K)), dim3(64), 0, (hipStream_t)stream, k);
    return launched();
}

extern "C" int md_kitti_eval_thresholds(MD_AOT_ARGS) {
    // in : sorted[Cn,3,K,Gt] f64, num_valid[Cn,3] i32 ; out: thresholds[Cn,3,K,41] f64, nthresh[Cn,3,K] i32
    Args a(MD_ARGS, 4, 4);
    a.tensor(0, KE_F64, 4); a.tensor(1, I32, 2); a.tensor(2, KE_F64, 4); a.tensor(3, I32, 3);
    if (int rc = a.rc()) return rc;
    const int64_t Cn = a.d(0, 0), K = a.d(0, 2), Gt = a.d(0, 3);
    a.require(Cn >= 1 && K >= 1 && Gt >= 0 && a.d(0, 1) == 3 && a.d(1, 0) == Cn && a.d(1, 1) == 3 && a.d(2, 0) == Cn && a.d(2, 1) == 3 &&
              a.d(2, 2) == K && a.d(2, 3) == KE_PTS && a.d(3, 0) == Cn && a.d(3, 1) == 3 && a.d(3, 2) == K);
    if (int rc = a.rc()) return rc;
    if (ke_too_large(0, Cn, K, Gt, 0, 0)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3})) return MD_ERR_ARG;
    if (aliased(params, 2, 4)) return MD_ERR_ARG;
    const int T = (int)(Cn * 3 * K);
    hipLaunchKernelGGL(ke_thresholds_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const double *)params[0],
                       (const int *)params[1], (double *)params[2], (int *)params[3], T, (int)K, Gt);
    return launched();
}

extern "C" int md_kitti_eval_stats(MD_AOT_ARGS) {
    // in : the eight operands of match_operands, thresholds[Cn,3,K,41] f64, nthresh[Cn,3,K] i32, gt_box[Gt,4] f64, gt_dc[Gt] u8,
    //      dt_box[Dt,4] f64, gt_alpha[Gt] f64, dt_alpha[Dt] f64
    // out: img_counts[Cn,3,K,41,I,3] i32, img_sim[Cn,3,K,41,I] f64, pr_counts[Cn,3,K,41,3] i32, pr_sim[Cn,3,K,41] f64
    Args a(MD_ARGS, 19, 19);
    const md_kitti_eval_stats_attrs *at = a.attrs<md_kitti_eval_stats_attrs>(extra);
    int64_t I, Cn, K, Gt, Dt, P;
    match_operands(a, I, Cn, K, Gt, Dt, P);
    a.tensor(8, KE_F64, 4); a.tensor(9, I32, 3); a.tensor(10, KE_F64, 2); a.tensor(11, U8, 1); a.tensor(12, KE_F64, 2); a.tensor(13, KE_F64, 1);
    a.tensor(14, KE_F64, 1); a.tensor(15, I32, 6); a.tensor(16, KE_F64, 5); a.tensor(17, I32, 5); a.tensor(18, KE_F64, 4);
    if (int rc = a.rc()) return rc;
    a.require(a.d(8, 0) == Cn && a.d(8, 1) == 3 && a.d(8, 2) == K && a.d(8, 3) == KE_PTS && a.d(9, 0) == Cn && a.d(9, 1) == 3 && a.d(9, 2) == K);
    a.require(a.d(10, 0) == Gt && a.d(10, 1) == 4 && a.d(11, 0) == Gt && a.d(12, 0) == Dt && a.d(12, 1) == 4 && a.d(13, 0) == Gt && a.d(14, 0) == Dt);
    for (int o = 15; o < 19; ++o) a.require(a.d(o, 0) == Cn && a.d(o, 1) == 3 && a.d(o, 2) == K && a.d(o, 3) == KE_PTS);
    a.require(a.d(15, 4) == I && a.d(15, 5) == 3 && a.d(16, 4) == I && a.d(17, 4) == 3);
    a.require(at->metric >= 0 && at->metric <= 2 && (at->compute_aos == 0 || at->compute_aos == 1));
    if (int rc = a.rc()) return rc;
    if (ke_too_large(I, Cn, K, Gt, Dt, P)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18})) return MD_ERR_ARG;
    if (aliased(params, 15, 19)) return MD_ERR_ARG;
    MatchArgs k;
    match_pointers(k, params, I, Cn, K, Gt, Dt, P);
    k.thresholds = (const double *)params[8]; k.nthresh = (const int *)params[9]; k.gt_box = (const double *)params[10];
    k.gt_dc = (const uint8_t *)params[11]; k.dt_box = (const double *)params[12]; k.gt_alpha = (const double *)params[13];
    k.dt_alpha = (const double *)params[14];
    k.img_counts = (int *)params[15]; k.img_sim = (double *)params[16]; k.pr_counts = (int *)params[17]; k.pr_sim = (double *)params[18];
    k.metric = at->metric; k.aos = at->compute_aos;
    const int T = (int)(Cn * 3 * K);
    hipStream_t s = (hipStream_t)stream;
    if (I > 0) hipLaunchKernelGGL(ke_stats_kernel, dim3((unsigned)(I * T)), dim3(64), 0, s, k);
    hipLaunchKernelGGL(ke_sum_kernel, dim3((unsigned)(T * KE_PTS)), dim3(256), 0, s, k);
    return launched();
}
