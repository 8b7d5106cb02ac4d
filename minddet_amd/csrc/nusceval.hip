// nusceval.hip -- the nuScenes detection evaluation on the device (include/minddet_hip_nusceval.h): from CenterPoint's (dets, count) and packed
// ground truth to the precision / confidence / true-positive error curves of the devkit's DetectionEval.  minddet_amd/nusc_eval.py states the
// same rules on the host and judges these.
//
//   md_nusc_rows             ne_rows_kernel    one workgroup per sample: every row to the global frame (two rows per lane, in registers), the
//                                              class-range filter, the class counts, and each row's place by counting the rows ahead of it
//                                              under (k, score descending, source row descending); keys in LDS
//   md_nusc_eval_match       ne_fill_kernel    dtm = -1, err = 0 everywhere (rows outside every cell keep that)
//                            ne_match_kernel   one wave per cell: ground truths over the lanes in chunks of 64 (<= 16 per lane, in registers),
//                                              one 16-bit taken set per threshold; per detection the distances once, then per threshold one
//                                              wave reduction on (distance, row)
//   md_nusc_eval_accumulate  ne_zero_kernel    tp_scan, m_conf, m_cum = 0 (positions outside every list keep that)
//                            ne_accum_kernel   one workgroup per (class, threshold): the integer scan of the matches over the class's list in
//                                              tiles of 256, the matches compacted behind it, their running error sums as five serial chains
//                                              (one lane per metric, tiles staged through LDS), then R binary searches per curve
// Float64 without contraction, no floating-point atomics, no memset, no scratch: every buffer is an operand.  A cell whose rows leave the
// operands is skipped, per-cell counts are clamped to the limits: nothing is read or written out of bounds.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#include "aot.h"
#include "../../include/minddet_hip_nusceval.h"
#include "workgroup.h"

namespace md {

static_assert(sizeof(md_nusc_rows_attrs) == 4 && sizeof(md_nusc_eval_attrs) == 4, "minddet_hip_nusceval.h: attribute struct layout");

constexpr const char *NE_F64 = "float64";
constexpr int NE_MAX_ROWS_SAMPLE = MD_NUSCEVAL_MAX_SAMPLE_DETS, NE_MAX_G = MD_NUSCEVAL_MAX_GTS, NE_MAX_K = MD_NUSCEVAL_MAX_CLASSES;
constexpr int NE_MAX_D = MD_NUSCEVAL_MAX_THRS, NE_MAX_R = MD_NUSCEVAL_MAX_RECS;
constexpr int NE_CHUNKS = NE_MAX_G / 64;        // ground truths per lane
static_assert(NE_CHUNKS == 16 && NE_MAX_G % 64 == 0, "the taken set of a threshold is one bit per chunk of a 16-bit mask");
static_assert(NE_MAX_ROWS_SAMPLE == 512 && NE_MAX_R <= 256 && NE_MAX_K <= 256, "two rows per lane; one lane per recall point / class in a workgroup of 256");

struct Quat { double w, x, y, z; };
struct Mat3 { double r[3][3]; };

__device__ __forceinline__ Quat ne_qmul(const Quat &a, const Quat &b) {
    Quat o;
    o.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    o.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    o.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
    o.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
    return o;
}
// the rotation matrix of the normalised quaternion
__device__ __forceinline__ Mat3 ne_matrix(const Quat &q) {
    const double n = sqrt(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z);
    const double w = q.w / n, x = q.x / n, y = q.y / n, z = q.z / n;
    Mat3 m;
    m.r[0][0] = 1 - 2 * (y * y + z * z); m.r[0][1] = 2 * (x * y - w * z); m.r[0][2] = 2 * (x * z + w * y);
    m.r[1][0] = 2 * (x * y + w * z); m.r[1][1] = 1 - 2 * (x * x + z * z); m.r[1][2] = 2 * (y * z - w * x);
    m.r[2][0] = 2 * (x * z - w * y); m.r[2][1] = 2 * (y * z + w * x); m.r[2][2] = 1 - 2 * (x * x + y * y);
    return m;
}
__device__ __forceinline__ void ne_rotate(const Mat3 &m, double *v) {
    const double a = v[0], b = v[1], c = v[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = (m.r[i][0] * a + m.r[i][1] * b) + m.r[i][2] * c;
}

// ---------------------------------------------------------------------------------------------------- rows
struct RowsArgs {
    const float *dets; const int *count; const double *pose; const int *label_to_k; const double *class_range; const int *attr_moving, *attr_still;
    double *dt_xyz, *dt_size, *dt_quat, *dt_vel, *dt_yaw, *dt_score; int *dt_cat, *dt_attr, *dt_rank, *dt_src, *dt_beg, *dt_cnt;
    int max_det, L, Kc, first;
};

__global__ __launch_bounds__(256) void ne_rows_kernel(RowsArgs a) {
    __shared__ int s_k[NE_MAX_ROWS_SAMPLE];
    __shared__ double s_sc[NE_MAX_ROWS_SAMPLE];
    __shared__ int s_beg[NE_MAX_K + 1], s_cnt[NE_MAX_K];
    const int tid = threadIdx.x, b = blockIdx.x, smp = a.first + b;
    int n = a.count[b];
    n = n < 0 ? 0 : (n > a.max_det ? a.max_det : n);
    const float *d = a.dets + (int64_t)b * a.max_det * 11;
    const double *ps = a.pose + (int64_t)b * 14;
    const Quat q_cs = {ps[0], ps[1], ps[2], ps[3]}, q_ego = {ps[7], ps[8], ps[9], ps[10]};
    const Mat3 m_cs = ne_matrix(q_cs), m_ego = ne_matrix(q_ego);
    double c[2][3], v[2][3], yaw[2];
    Quat q[2];
    int attr[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int r = tid + 256 * it;
        int k = -1;
        double s = 0.0;
        c[it][0] = c[it][1] = c[it][2] = v[it][0] = v[it][1] = v[it][2] = yaw[it] = 0.0;
        q[it] = Quat{0.0, 0.0, 0.0, 0.0};
        attr[it] = 0;
        if (r < n) {
            const float *row = d + r * 11;
            const float yf = (-row[8]) - (float)(M_PI / 2);
            const double h = (double)yf / 2;
            Quat o = {cos(h), 0.0, 0.0, sin(h)};
            c[it][0] = (double)row[0]; c[it][1] = (double)row[1]; c[it][2] = (double)row[2];
            v[it][0] = (double)row[6]; v[it][1] = (double)row[7]; v[it][2] = 0.0;
            ne_rotate(m_cs, c[it]);
            c[it][0] += ps[4]; c[it][1] += ps[5]; c[it][2] += ps[6];
            o = ne_qmul(q_cs, o);
            ne_rotate(m_cs, v[it]);
            ne_rotate(m_ego, c[it]);
            c[it][0] += ps[11]; c[it][1] += ps[12]; c[it][2] += ps[13];
            o = ne_qmul(q_ego, o);
            ne_rotate(m_ego, v[it]);
            q[it] = o;
            const Mat3 mo = ne_matrix(o);
            yaw[it] = atan2(mo.r[1][0], mo.r[0][0]);
            const float lab = row[10];
            const double sc = (double)row[9];
            if (lab > -1.0f && lab < (float)a.L && sc == sc) {    // int(label) lies in [0, L); a NaN fails both
                const int kv = a.label_to_k[(int)lab];
                if (kv >= 0 && kv < a.Kc) {
                    const double ex = c[it][0] - ps[11], ey = c[it][1] - ps[12];
                    if (sqrt(ex * ex + ey * ey) < a.class_range[kv]) {
                        k = kv;
                        s = sc;
                        attr[it] = sqrt(v[it][0] * v[it][0] + v[it][1] * v[it][1]) > 0.2 ? a.attr_moving[kv] : a.attr_still[kv];
                    }
                }
            }
        }
        if (r < NE_MAX_ROWS_SAMPLE) { s_k[r] = k; s_sc[r] = s; }
    }
    __syncthreads();
    for (int k = tid; k < a.Kc; k += 256) {
        int cn = 0;
        for (int r = 0; r < n; ++r) cn += s_k[r] == k;
        s_cnt[k] = cn;
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int k = 0; k < a.Kc; ++k) { s_beg[k] = acc; acc += s_cnt[k]; }
        s_beg[a.Kc] = acc;
    }
    __syncthreads();
    const int64_t row0 = (int64_t)smp * a.max_det;
    for (int k = tid; k < a.Kc; k += 256) {
        a.dt_beg[(int64_t)smp * a.Kc + k] = (int)(row0 + s_beg[k]);
        a.dt_cnt[(int64_t)smp * a.Kc + k] = s_cnt[k];
    }
    for (int p = s_beg[a.Kc] + tid; p < a.max_det; p += 256) {     // the unused tail of the sample's block
        const int64_t at = row0 + p;
        for (int i = 0; i < 3; ++i) { a.dt_xyz[at * 3 + i] = 0.0; a.dt_size[at * 3 + i] = 0.0; }
        for (int i = 0; i < 4; ++i) a.dt_quat[at * 4 + i] = 0.0;
        a.dt_vel[at * 2] = 0.0; a.dt_vel[at * 2 + 1] = 0.0; a.dt_yaw[at] = 0.0; a.dt_score[at] = 0.0;
        a.dt_cat[at] = a.Kc; a.dt_attr[at] = 0; a.dt_rank[at] = 0; a.dt_src[at] = -1;
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int r = tid + 256 * it;
        if (r >= n) continue;
        const int k = s_k[r];
        if (k < 0) continue;
        const double s = s_sc[r];
        int rank = 0;                                         // the rows of the cell ahead of r: a higher score, or an equal one from a later row
        for (int o = 0; o < n; ++o)
            if (s_k[o] == k) rank += (s_sc[o] > s) || (s_sc[o] == s && o > r);
        const int64_t at = row0 + s_beg[k] + rank;
        const float *row = d + r * 11;
        for (int i = 0; i < 3; ++i) { a.dt_xyz[at * 3 + i] = c[it][i]; a.dt_size[at * 3 + i] = (double)row[3 + i]; }
        a.dt_quat[at * 4] = q[it].w; a.dt_quat[at * 4 + 1] = q[it].x; a.dt_quat[at * 4 + 2] = q[it].y; a.dt_quat[at * 4 + 3] = q[it].z;
        a.dt_vel[at * 2] = v[it][0]; a.dt_vel[at * 2 + 1] = v[it][1]; a.dt_yaw[at] = yaw[it]; a.dt_score[at] = s;
        a.dt_cat[at] = k; a.dt_attr[at] = attr[it]; a.dt_rank[at] = rank; a.dt_src[at] = r;
    }
}

// ---------------------------------------------------------------------------------------------------- matching
struct MatchArgs {
    const int *gt_beg, *gt_cnt, *dt_beg, *dt_cnt;
    const double *gt_xy, *gt_size, *gt_yaw, *gt_vel; const int *gt_attr;
    const double *dt_xyz, *dt_size, *dt_yaw, *dt_vel; const int *dt_attr; const double *dist_thr, *period;
    int *dtm; double *err; int *cell_ngt;
    int64_t Gt, Dt;
    int C, Kc, D, tp;
};

__global__ __launch_bounds__(256) void ne_fill_kernel(int *dtm, int64_t n_dtm, double *err, int64_t n_err) {
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t i = i0; i < n_dtm; i += step) dtm[i] = -1;
    for (int64_t i = i0; i < n_err; i += step) err[i] = 0.0;
}

// Python's float %: fmod moved to the sign of the divisor
__device__ __forceinline__ double ne_pymod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0) != (m < 0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

__global__ __launch_bounds__(64) void ne_match_kernel(MatchArgs a) {
    const int lane = threadIdx.x, cell = blockIdx.x, k = cell % a.Kc;
    const int64_t g0 = a.gt_beg[cell], gc = a.gt_cnt[cell], d0 = a.dt_beg[cell], dc = a.dt_cnt[cell];
    const bool gok = g0 >= 0 && gc >= 0 && g0 + gc <= a.Gt, dok = d0 >= 0 && dc >= 0 && d0 + dc <= a.Dt;
    const int G = gok ? (int)(gc < NE_MAX_G ? gc : NE_MAX_G) : 0, Dn = dok ? (int)(dc < NE_MAX_ROWS_SAMPLE ? dc : NE_MAX_ROWS_SAMPLE) : 0;
    if (lane == 0) a.cell_ngt[cell] = G;
    if (Dn == 0 || G == 0) return;                            // nothing to match: the fill stands
    double gx[NE_CHUNKS], gy[NE_CHUNKS];
    const int nch = (G + 63) >> 6;
#pragma unroll
    for (int ch = 0; ch < NE_CHUNKS; ++ch) {
        const int g = lane + 64 * ch;
        gx[ch] = gy[ch] = 0.0;
        if (g < G) { gx[ch] = a.gt_xy[(g0 + g) * 2]; gy[ch] = a.gt_xy[(g0 + g) * 2 + 1]; }
    }
    unsigned taken[NE_MAX_D];
#pragma unroll
    for (int t = 0; t < NE_MAX_D; ++t) taken[t] = 0;
    const double inf = __builtin_inf();
    for (int d = 0; d < Dn; ++d) {
        const int64_t row = d0 + d;
        const double px = a.dt_xyz[row * 3], py = a.dt_xyz[row * 3 + 1];
        double dist[NE_CHUNKS];
#pragma unroll
        for (int ch = 0; ch < NE_CHUNKS; ++ch) {
            dist[ch] = inf;
            if (ch < nch && lane + 64 * ch < G) {
                const double dx = px - gx[ch], dy = py - gy[ch];
                dist[ch] = sqrt(dx * dx + dy * dy);
            }
        }
#pragma unroll
        for (int t = 0; t < NE_MAX_D; ++t) {
            if (t >= a.D) continue;
            double bd = inf;
            int bi = -1;
#pragma unroll
            for (int ch = 0; ch < NE_CHUNKS; ++ch)
                if (!(taken[t] >> ch & 1) && dist[ch] < bd) { bd = dist[ch]; bi = lane + 64 * ch; }      // strict: the first row on equal distance
            for (int off = 32; off > 0; off >>= 1) {          // every lane ends with the winner
                const double od = __shfl_xor(bd, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (oi >= 0 && (bi < 0 || od < bd || (od == bd && oi < bi))) { bd = od; bi = oi; }
            }
            const bool hit = bi >= 0 && bd < a.dist_thr[t];
            if (hit && (bi & 63) == lane) taken[t] |= 1u << (bi >> 6);
            if (lane == 0 && hit) {
                const int64_t g = g0 + bi;
                a.dtm[(int64_t)t * a.Dt + row] = (int)g;
                if (t == a.tp) {
                    const double *sa = a.gt_size + g * 3, *sr = a.dt_size + row * 3;
                    const double m0 = sa[0] < sr[0] ? sa[0] : sr[0], m1 = sa[1] < sr[1] ? sa[1] : sr[1], m2 = sa[2] < sr[2] ? sa[2] : sr[2];
                    const double va = (sa[0] * sa[1]) * sa[2], vr = (sr[0] * sr[1]) * sr[2], inter = (m0 * m1) * m2;
                    const double per = a.period[k], pi = 3.141592653589793;
                    double df = ne_pymod((a.gt_yaw[g] - a.dt_yaw[row]) + per / 2, per) - per / 2;
                    if (df > pi) df = df - 2 * pi;
                    const double dvx = a.gt_vel[g * 2] - a.dt_vel[row * 2], dvy = a.gt_vel[g * 2 + 1] - a.dt_vel[row * 2 + 1];
                    const int ga = a.gt_attr[g];
                    double *e = a.err + row * 5;
                    e[0] = bd;
                    e[1] = 1 - inter / ((va + vr) - inter);
                    e[2] = fabs(df);
                    e[3] = sqrt(dvx * dvx + dvy * dvy);
                    e[4] = ga < 0 ? __builtin_nan("") : 1 - (double)(ga == a.dt_attr[row]);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- accumulate
struct AccumArgs {
    const int *order, *cat_off; const double *dt_score; const int *dtm; const double *err; const int *cell_ngt; const double *rec_thr;
    double *precision, *confidence, *tp_err; int *n_gt, *n_match, *tp_scan; double *m_conf, *m_cum;
    int64_t Dt;
    int C, Kc, D, R, tp;
};

__global__ __launch_bounds__(256) void ne_zero_kernel(int *tp_scan, int64_t n_scan, double *m_conf, int64_t n_conf, double *m_cum, int64_t n_cum) {
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    for (int64_t i = i0; i < n_scan; i += step) tp_scan[i] = 0;
    for (int64_t i = i0; i < n_conf; i += step) m_conf[i] = 0.0;
    for (int64_t i = i0; i < n_cum; i += step) m_cum[i] = 0.0;
}

// np.interp for one x: xp(j) ascending and fp(j) for j in [0, n), n >= 1
template <typename XP, typename FP> __device__ __forceinline__ double ne_interp(double x, int n, XP xp, FP fp, bool has_right, double right) {
    if (x != x) return x;
    int lo = 0, hi = n;                                       // the number of j with xp(j) <= x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xp(mid) <= x) lo = mid + 1; else hi = mid;
    }
    const int j = lo - 1;
    if (j < 0) return fp(0);
    if (j == n - 1) return (has_right && x > xp(j)) ? right : fp(j);
    const double xj = xp(j), fj = fp(j);
    if (xj == x) return fj;
    const double x1 = xp(j + 1), f1 = fp(j + 1);
    const double slope = (f1 - fj) / (x1 - xj);
    double v = slope * (x - xj) + fj;
    if (v != v) {
        v = slope * (x - x1) + f1;
        if (v != v && fj == f1) v = fj;
    }
    return v;
}

__global__ __launch_bounds__(256) void ne_accum_kernel(AccumArgs a) {
    __shared__ double s_e[5][256], s_conf[NE_MAX_R];
    __shared__ int wsum[4], red[4];
    const int tid = threadIdx.x, k = blockIdx.x / a.D, d = blockIdx.x % a.D, I = a.C / a.Kc;
    const bool tp_blk = d == a.tp;
    int ngt = 0;
    for (int i = tid; i < I; i += 256) ngt += a.cell_ngt[(int64_t)i * a.Kc + k];
    ngt = block_count(ngt, red);
    if (tid == 0 && d == 0) a.n_gt[k] = ngt;
    int64_t beg = a.cat_off[k], end = a.cat_off[k + 1];
    if (beg < 0 || end > a.Dt || end < beg) beg = end = 0;    // a list that leaves the operand is skipped
    const int n = (int)(end - beg);
    int ctp = 0, valid[5] = {0, 0, 0, 0, 0};
    for (int64_t base = beg; base < end; base += 256) {
        const int64_t j = base + tid;
        int tpf = 0;
        int64_t row = -1;
        if (j < end) {
            row = a.order[j];
            if (row < 0 || row >= a.Dt) row = -1;
            else tpf = a.dtm[(int64_t)d * a.Dt + row] >= 0;
        }
        int all;
        const int inc = ctp + block_exclusive_scan<4>(tpf, wsum, all) + tpf;
        if (j < end) a.tp_scan[(int64_t)d * a.Dt + j] = inc;
        if (tp_blk) {
            double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            if (tpf) {
                const int64_t pos = beg + inc - 1;            // inc - 1 <= j - beg: inside the class's list
                a.m_conf[pos] = a.dt_score[row];
#pragma unroll
                for (int m = 0; m < 5; ++m) { e[m] = a.err[row * 5 + m]; a.m_cum[(int64_t)m * a.Dt + pos] = e[m]; }
            }
#pragma unroll
            for (int m = 0; m < 5; ++m) valid[m] += block_count(tpf && e[m] == e[m], red);
        }
        ctp += all;
    }
    const int nm = ctp;
    if (tid == 0) a.n_match[k * a.D + d] = nm;
    const bool none = ngt <= 0 || nm == 0;
    __syncthreads();
    if (tp_blk && !none) {                                    // the running means: np.cumsum's order, one lane per metric
        double sum = 0.0;
        int cnt = 0;
        for (int base = 0; base < nm; base += 256) {
            const int n_in = nm - base < 256 ? nm - base : 256;
            if (tid < n_in)
#pragma unroll
                for (int m = 0; m < 5; ++m) s_e[m][tid] = a.m_cum[(int64_t)m * a.Dt + beg + base + tid];
            __syncthreads();
            if (tid < 5) {
                const bool all_nan = valid[tid] == 0;
                for (int i = 0; i < n_in; ++i) {
                    const double v = s_e[tid][i];
                    const bool nan = v != v;
                    sum += nan ? 0.0 : v;
                    cnt += !nan;
                    s_e[tid][i] = all_nan ? 1.0 : (cnt > 0 ? sum / (double)cnt : 0.0);
                }
            }
            __syncthreads();
            if (tid < n_in)
#pragma unroll
                for (int m = 0; m < 5; ++m) a.m_cum[(int64_t)m * a.Dt + beg + base + tid] = s_e[m][tid];
            __syncthreads();
        }
    }
    const double dngt = (double)ngt;
    const int *scan = a.tp_scan + (int64_t)d * a.Dt + beg;
    if (tid < a.R) {
        double pr = 0.0, cf = 0.0;
        if (!none) {
            const double x = a.rec_thr[tid];
            auto rec = [&](int j) { return (double)scan[j] / dngt; };
            pr = ne_interp(x, n, rec, [&](int j) { const double t = (double)scan[j], f = (double)(j + 1 - scan[j]); return t / (f + t); }, true, 0.0);
            cf = ne_interp(x, n, rec, [&](int j) { const int64_t row = a.order[beg + j]; return row >= 0 && row < a.Dt ? a.dt_score[row] : 0.0; }, true, 0.0);
        }
        const int64_t at = ((int64_t)k * a.D + d) * a.R + tid;
        a.precision[at] = pr;
        a.confidence[at] = cf;
        s_conf[tid] = cf;
    }
    __syncthreads();
    if (tp_blk) {
        for (int idx = tid; idx < 5 * a.R; idx += 256) {
            const int m = idx / a.R, r = idx % a.R;
            double v = 1.0;
            if (!none) {
                const double *mc = a.m_conf + beg, *cm = a.m_cum + (int64_t)m * a.Dt + beg;
                v = ne_interp(s_conf[r], nm, [&](int j) { return mc[nm - 1 - j]; }, [&](int j) { return cm[nm - 1 - j]; }, false, 0.0);
            }
            a.tp_err[((int64_t)k * 5 + m) * a.R + r] = v;
        }
    }
}

// the limits every op holds its extents to
static bool ne_too_large(int64_t C, int64_t Kc, int64_t Gt, int64_t Dt, int64_t D, int64_t R) {
    return C >= MD_NUSCEVAL_MAX_CELLS || Kc > MD_NUSCEVAL_MAX_CLASSES || Gt > MD_NUSCEVAL_MAX_ROWS || Dt > MD_NUSCEVAL_MAX_ROWS ||
           D > MD_NUSCEVAL_MAX_THRS || R > MD_NUSCEVAL_MAX_RECS;
}

}  // namespace md

using namespace md;

extern "C" int md_nusc_rows(MD_AOT_ARGS) {
    // in : dets[B,max_det,11] f32, count[B] i32, pose[B,14] f64, label_to_k[L] i32, class_range[Kc] f64, attr_moving[Kc] i32, attr_still[Kc] i32
    // out: dt_xyz[Dt,3], dt_size[Dt,3], dt_quat[Dt,4], dt_vel[Dt,2], dt_yaw[Dt], dt_score[Dt] f64, dt_cat, dt_attr, dt_rank, dt_src [Dt] i32,
    //      dt_beg[C], dt_cnt[C] i32
    Args a(MD_ARGS, 19, 19);
    const md_nusc_rows_attrs *at = a.attrs<md_nusc_rows_attrs>(extra);
    a.tensor(0, F32, 3); a.tensor(1, I32, 1); a.tensor(2, NE_F64, 2); a.tensor(3, I32, 1); a.tensor(4, NE_F64, 1); a.tensor(5, I32, 1); a.tensor(6, I32, 1);
    a.tensor(7, NE_F64, 2); a.tensor(8, NE_F64, 2); a.tensor(9, NE_F64, 2); a.tensor(10, NE_F64, 2); a.tensor(11, NE_F64, 1); a.tensor(12, NE_F64, 1);
    for (int i = 13; i < 19; ++i) a.tensor(i, I32, 1);
    if (int rc = a.rc()) return rc;
    const int64_t B = a.d(0, 0), max_det = a.d(0, 1), L = a.d(3, 0), Kc = a.d(4, 0), Dt = a.d(7, 0), C = a.d(17, 0);
    a.require(B >= 0 && max_det >= 1 && a.d(0, 2) == 11 && a.d(1, 0) == B && a.d(2, 0) == B && a.d(2, 1) == 14 && L >= 1 && Kc >= 1 && Dt >= 1 && C >= 1);
    a.require(a.d(5, 0) == Kc && a.d(6, 0) == Kc && a.d(7, 1) == 3 && a.d(8, 0) == Dt && a.d(8, 1) == 3 && a.d(9, 0) == Dt && a.d(9, 1) == 4 &&
              a.d(10, 0) == Dt && a.d(10, 1) == 2);
    for (int i = 11; i < 17; ++i) a.require(a.d(i, 0) == Dt);
    a.require(a.d(18, 0) == C);
    if (int rc = a.rc()) return rc;
    a.require(Dt % max_det == 0 && C % Kc == 0 && C / Kc == Dt / max_det);
    if (int rc = a.rc()) return rc;
    const int64_t I = Dt / max_det;
    a.require(at->first_sample >= 0 && (int64_t)at->first_sample + B <= I);
    if (int rc = a.rc()) return rc;
    if (max_det > MD_NUSCEVAL_MAX_SAMPLE_DETS || L > MD_NUSCEVAL_MAX_LABELS || ne_too_large(C, Kc, 0, Dt, 0, 0)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18})) return MD_ERR_ARG;
    if (aliased(params, 7, 19)) return MD_ERR_ARG;
    if (B == 0) return MD_OK;
    RowsArgs k;
    k.dets = (const float *)params[0]; k.count = (const int *)params[1]; k.pose = (const double *)params[2]; k.label_to_k = (const int *)params[3];
    k.class_range = (const double *)params[4]; k.attr_moving = (const int *)params[5]; k.attr_still = (const int *)params[6];
    k.dt_xyz = (double *)params[7]; k.dt_size = (double *)params[8]; k.dt_quat = (double *)params[9]; k.dt_vel = (double *)params[10];
    k.dt_yaw = (double *)params[11]; k.dt_score = (double *)params[12]; k.dt_cat = (int *)params[13]; k.dt_attr = (int *)params[14];
    k.dt_rank = (int *)params[15]; k.dt_src = (int *)params[16]; k.dt_beg = (int *)params[17]; k.dt_cnt = (int *)params[18];
    k.max_det = (int)max_det; k.L = (int)L; k.Kc = (int)Kc; k.first = at->first_sample;
    hipLaunchKernelGGL(ne_rows_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, k);
    return launched();
}

extern "C" int md_nusc_eval_match(MD_AOT_ARGS) {
    // in : gt_beg, gt_cnt, dt_beg, dt_cnt [C] i32, gt_xy[Gt,2], gt_size[Gt,3], gt_yaw[Gt], gt_vel[Gt,2] f64, gt_attr[Gt] i32, dt_xyz[Dt,3], dt_size[Dt,3],
    //      dt_yaw[Dt], dt_vel[Dt,2] f64, dt_attr[Dt] i32, dist_thr[D] f64, period[Kc] f64 ; out: dtm[D,Dt] i32, err[Dt,5] f64, cell_ngt[C] i32
    Args a(MD_ARGS, 19, 19);
    const md_nusc_eval_attrs *at = a.attrs<md_nusc_eval_attrs>(extra);
    a.tensor(0, I32, 1); a.tensor(1, I32, 1); a.tensor(2, I32, 1); a.tensor(3, I32, 1); a.tensor(4, NE_F64, 2); a.tensor(5, NE_F64, 2); a.tensor(6, NE_F64, 1);
    a.tensor(7, NE_F64, 2); a.tensor(8, I32, 1); a.tensor(9, NE_F64, 2); a.tensor(10, NE_F64, 2); a.tensor(11, NE_F64, 1); a.tensor(12, NE_F64, 2);
    a.tensor(13, I32, 1); a.tensor(14, NE_F64, 1); a.tensor(15, NE_F64, 1); a.tensor(16, I32, 2); a.tensor(17, NE_F64, 2); a.tensor(18, I32, 1);
    if (int rc = a.rc()) return rc;
    const int64_t C = a.d(0, 0), Gt = a.d(4, 0), Dt = a.d(9, 0), D = a.d(14, 0), Kc = a.d(15, 0);
    a.require(C >= 1 && Gt >= 0 && Dt >= 0 && D >= 1 && Kc >= 1 && a.d(1, 0) == C && a.d(2, 0) == C && a.d(3, 0) == C && a.d(4, 1) == 2);
    a.require(a.d(5, 0) == Gt && a.d(5, 1) == 3 && a.d(6, 0) == Gt && a.d(7, 0) == Gt && a.d(7, 1) == 2 && a.d(8, 0) == Gt && a.d(9, 1) == 3);
    a.require(a.d(10, 0) == Dt && a.d(10, 1) == 3 && a.d(11, 0) == Dt && a.d(12, 0) == Dt && a.d(12, 1) == 2 && a.d(13, 0) == Dt);
    a.require(a.d(16, 0) == D && a.d(16, 1) == Dt && a.d(17, 0) == Dt && a.d(17, 1) == 5 && a.d(18, 0) == C);
    if (int rc = a.rc()) return rc;
    a.require(C % Kc == 0 && at->tp_index >= 0 && at->tp_index < D);
    if (int rc = a.rc()) return rc;
    if (ne_too_large(C, Kc, Gt, Dt, D, 0)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18})) return MD_ERR_ARG;
    if (aliased(params, 16, 19)) return MD_ERR_ARG;
    MatchArgs k;
    k.gt_beg = (const int *)params[0]; k.gt_cnt = (const int *)params[1]; k.dt_beg = (const int *)params[2]; k.dt_cnt = (const int *)params[3];
    k.gt_xy = (const double *)params[4]; k.gt_size = (const double *)params[5]; k.gt_yaw = (const double *)params[6]; k.gt_vel = (const double *)params[7];
    k.gt_attr = (const int *)params[8]; k.dt_xyz = (const double *)params[9]; k.dt_size = (const double *)params[10]; k.dt_yaw = (const double *)params[11];
    k.dt_vel = (const double *)params[12]; k.dt_attr = (const int *)params[13]; k.dist_thr = (const double *)params[14]; k.period = (const double *)params[15];
    k.dtm = (int *)params[16]; k.err = (double *)params[17]; k.cell_ngt = (int *)params[18];
    k.Gt = Gt; k.Dt = Dt; k.C = (int)C; k.Kc = (int)Kc; k.D = (int)D; k.tp = at->tp_index;
    hipStream_t s = (hipStream_t)stream;
    if (Dt > 0) hipLaunchKernelGGL(ne_fill_kernel, dim3(grid1d((size_t)(D * Dt))), dim3(256), 0, s, k.dtm, D * Dt, k.err, Dt * 5);
    hipLaunchKernelGGL(ne_match_kernel, dim3((unsigned)C), dim3(64), 0, s, k);
    return launched();
}

extern "C" int md_nusc_eval_accumulate(MD_AOT_ARGS) {
    // in : order[Dt] i32, cat_off[Kc+1] i32, dt_score[Dt] f64, dtm[D,Dt] i32, err[Dt,5] f64, cell_ngt[C] i32, rec_thr[R] f64
    // out: precision[Kc,D,R], confidence[Kc,D,R], tp_err[Kc,5,R] f64, n_gt[Kc], n_match[Kc,D], tp_scan[D,Dt] i32, m_conf[Dt], m_cum[5,Dt] f64
    Args a(MD_ARGS, 15, 15);
    const md_nusc_eval_attrs *at = a.attrs<md_nusc_eval_attrs>(extra);
    a.tensor(0, I32, 1); a.tensor(1, I32, 1); a.tensor(2, NE_F64, 1); a.tensor(3, I32, 2); a.tensor(4, NE_F64, 2); a.tensor(5, I32, 1); a.tensor(6, NE_F64, 1);
    a.tensor(7, NE_F64, 3); a.tensor(8, NE_F64, 3); a.tensor(9, NE_F64, 3); a.tensor(10, I32, 1); a.tensor(11, I32, 2); a.tensor(12, I32, 2);
    a.tensor(13, NE_F64, 1); a.tensor(14, NE_F64, 2);
    if (int rc = a.rc()) return rc;
    const int64_t Dt = a.d(0, 0), Kc = a.d(1, 0) - 1, D = a.d(3, 0), C = a.d(5, 0), R = a.d(6, 0);
    a.require(Dt >= 0 && Kc >= 1 && D >= 1 && C >= 1 && R >= 1 && a.d(2, 0) == Dt && a.d(3, 1) == Dt && a.d(4, 0) == Dt && a.d(4, 1) == 5);
    a.require(a.d(7, 0) == Kc && a.d(7, 1) == D && a.d(7, 2) == R && a.d(8, 0) == Kc && a.d(8, 1) == D && a.d(8, 2) == R && a.d(9, 0) == Kc &&
              a.d(9, 1) == 5 && a.d(9, 2) == R);
    a.require(a.d(10, 0) == Kc && a.d(11, 0) == Kc && a.d(11, 1) == D && a.d(12, 0) == D && a.d(12, 1) == Dt && a.d(13, 0) == Dt && a.d(14, 0) == 5 &&
              a.d(14, 1) == Dt);
    if (int rc = a.rc()) return rc;
    a.require(C % Kc == 0 && at->tp_index >= 0 && at->tp_index < D);
    if (int rc = a.rc()) return rc;
    if (ne_too_large(C, Kc, 0, Dt, D, R)) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14})) return MD_ERR_ARG;
    if (aliased(params, 7, 15)) return MD_ERR_ARG;
    AccumArgs k;
    k.order = (const int *)params[0]; k.cat_off = (const int *)params[1]; k.dt_score = (const double *)params[2]; k.dtm = (const int *)params[3];
    k.err = (const double *)params[4]; k.cell_ngt = (const int *)params[5]; k.rec_thr = (const double *)params[6];
    k.precision = (double *)params[7]; k.confidence = (double *)params[8]; k.tp_err = (double *)params[9]; k.n_gt = (int *)params[10];
    k.n_match = (int *)params[11]; k.tp_scan = (int *)params[12]; k.m_conf = (double *)params[13]; k.m_cum = (double *)params[14];
    k.Dt = Dt; k.C = (int)C; k.Kc = (int)Kc; k.D = (int)D; k.R = (int)R; k.tp = at->tp_index;
    hipStream_t s = (hipStream_t)stream;
    if (Dt > 0) hipLaunchKernelGGL(ne_zero_kernel, dim3(grid1d((size_t)(D * Dt))), dim3(256), 0, s, k.tp_scan, D * Dt, k.m_conf, Dt, k.m_cum, 5 * Dt);
    hipLaunchKernelGGL(ne_accum_kernel, dim3((unsigned)(Kc * D)), dim3(256), 0, s, k);
    return launched();
}
