// convbwd.hip -- weight gradient of a pointwise (1x1) convolution on the device (include/minddet_hip_train.h): md_conv1x1_bwd_weight,
// dw[o, i] = sum_p dy[p, o] x[p, i] and db[o] = sum_p dy[p, o] over the P = N H W pixels of an NHWC bf16 activation and the fp32
// gradient a md_*_loss_grad wrote.
//
// The reduction index is the pixel, the slow axis of both operands in memory.  A bf16 MFMA holds eight consecutive reduction indices in
// one lane's fragment, which would ask for a transpose of both operands; the fp32 MFMA (v_mfma_f32_16x16x4_f32) holds ONE per lane and
// spreads its four over the lane quarters (A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15]).  So lane (c, q) of a
// wave loads, for pixel q of a group of four, the 16 bytes x[p][128 g + 8 c .. + 7] as they lie in memory and feeds element j to MFMA j
// of eight: column c of MFMA j is channel 128 g + 8 c + j, a permutation the store undoes.  dy is one 4-byte load per 16 rows.  No
// transpose, no LDS on the way in, x read once by each workgroup row (blockIdx.z: 64 output channels), dy with all 24 bits.
// The fp32 MFMA runs at 1 / 16 of the bf16 rate: at cin 384, cout 20 .. 32 the products take about as long as reading x from HBM.
//
// Two launches, no atomics, no workgroup waits on another:
//   conv1x1_wgrad_kernel<MT>     grid (slabs, ceil(cin / 128), ceil(cout / 16 MT)); 4 waves, wave w takes pixel groups 4 s + w of the slab
//                                (the workgroup walks 16 consecutive pixels per step), loads four steps ahead; the waves' accumulators
//                                are added in order through LDS; wave 0 stores the [16 MT][128] block of the slab to the workspace
//   conv1x1_wgrad_sum_kernel     per element of dw / db: 8 interleaved chains over the slabs, then the chains in order; padding +0.0
// The order of every addition is fixed by P alone (the header states the longest chain, L(P)).
//
// md_conv_bwd_weight (include/minddet_hip_convbwd.h) is the same two launches for a k x k conv, k = 1 or 3: (tap, channel) is one virtual
// column axis of k k cin columns, an 8-channel chunk lies inside one tap (cin % 8 == 0), so lane group c owns one tap's chunk and loads
// its own shifted pixel x[p + d_t] under its own in-image predicate (K = 3 instantiation; K = 1 is the kernel above, unchanged).  The
// summing launch maps an element of dw to its virtual column (both K orders of a pack) and writes +0.0 outside the layer's blocks.
//
// md_conv1x1_bwd_data: dx[p, i] = sum_o dy[p, o] w[o, i], optionally through a ReLU mask.  conv1x1_dgrad_kernel, grid (ceil(P / 256),
// ceil(cin / 128)): the workgroup keeps the [cout][128] tile of w (bf16) in LDS, each wave takes 16 pixels per step as the MFMA's rows, o
// as its reduction index (lane (c, q) loads dy[pixel c][4 s + q]: the fast axis of dy, no transpose), eight MFMAs per step and o-quad for
// the eight channels of lane group c; the lane then holds eight consecutive channels of four pixels and stores them as two 16-byte rows.
//
// md_conv2d_grouped_bwd_weight / _bwd_data (include/minddet_hip_groupedbwd.h) carry the gradient through md_conv2d_grouped (grouped.hip):
// the weight gradient is wgrad_body<1, K> with the group as blockIdx.z (grouped_wgrad_kernel) and a summing launch that finds an element's
// group by its row; the data gradient is grouped_dgrad_kernel, the pointwise form with (tap, o) as the reduction index and each lane's own
// shifted pixel of dy, 64 channels (one group) per 16 lanes.
#include <math.h>

#include "aot.h"
#include "device.h"
#include "../../include/minddet_hip_groupedbwd.h"

#pragma clang fp contract(off)

namespace md {

static_assert(sizeof(md_conv1x1_bwd_attrs) == 5 * 4, "minddet_hip_train.h: attribute struct layout");
static_assert(sizeof(md_conv_bwd_attrs) == 24 * 4 && sizeof(md_conv1x1_bwd_data_attrs) == 6 * 4, "minddet_hip_convbwd.h: attribute struct layout");
static_assert(MD_CONV_BWD_MAX_CIN_K1 == MD_CONV1X1_BWD_MAX_CIN && MD_CONV_BWD_MAX_COUT == MD_CONV1X1_BWD_MAX_COUT, "one kernel, one set of limits");

constexpr int WG_GROUP = 128;   // channels of x per workgroup column: 16 lanes x 8 bf16 = one 16-byte load per lane
constexpr int WG_RING = 4;      // pixel groups a wave loads ahead of its MFMAs
constexpr int WG_WAYS = MD_CONV1X1_BWD_SUM_WAYS;

struct WgParams {
    int P, S, n_slabs, cin, cout, R;      // R: rows of a partial block = cout rounded up to 16
    int Cx, Cy, x_c_off, dy_c_off, xvec;  // xvec: every 8-channel chunk of x the layer reads is 16-byte aligned
    int rows, kpad, rowsb;                // extents of dw and db (rowsb 0: no db)
    // md_conv_bwd_weight: KK = taps cin virtual columns (taps = 1: KK = cin), the map's extents, dw's column order and the live blocks
    int KK, taps, H, W, korder, n_blocks;
    md_conv_bwd_block blk[MD_CONV_BWD_MAX_BLOCKS];
};

// x[p][ch .. ch + 7] as four packed words; zero where the lane has no pixel or no channels
__device__ __forceinline__ u32x4 wg_load_x(const uint16_t *__restrict__ x, size_t elem, bool ok, int xvec) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (ok) {
        if (xvec) {
            v = *(const u32x4 *)(x + elem);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (unsigned)x[elem + 2 * k] | ((unsigned)x[elem + 2 * k + 1] << 16);
        }
    }
    return v;
}

// the body of the first launch; ob: the first output channel of the workgroup's 16 MT rows
template <int MT, int K>
__device__ __forceinline__ void wgrad_body(const uint16_t *__restrict__ x, const float *__restrict__ dy, const WgParams &p,
                                           float *__restrict__ ws_dw, float *__restrict__ ws_db, const int ob) {
    __shared__ float s_acc[MT * 8 * 4 * 64];   // one wave's accumulators, [(m 8 + j) 4 + reg][lane]
    __shared__ float s_db[4][MT * 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int slab = blockIdx.x, ch = blockIdx.y * WG_GROUP + 8 * c;
    const long long p0 = (long long)slab * p.S;
    const int pend = (int)min((long long)p.P, p0 + p.S);   // one past the slab's last pixel
    const int ncol = K == 1 ? p.cin : p.KK;                // columns of a partial block; K = 3: ch is the virtual column tap cin + channel
    const bool chok = ch < ncol;                           // (cin % 8 == 0: a chunk is inside the layer, and inside one tap, or outside it)
    const int tap = K == 1 ? 0 : ch / p.cin, ddy = K == 1 ? 0 : tap / K - K / 2, ddx = K == 1 ? 0 : tap % K - K / 2;
    bool rowok[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) rowok[m] = ob + 16 * m + c < p.cout;
    const uint16_t *xs = x + p.x_c_off + (ch - tap * p.cin);
    const float *ds = dy + p.dy_c_off + ob + c;

    f32x4 acc[MT][8];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float dbacc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) dbacc[m] = 0.f;

    // step s of this wave: pixel p0 + 16 s + 4 wave + q
    const int steps = (int)((pend - p0 + 15) / 16);
    u32x4 xr[WG_RING];
    float ar[WG_RING][MT];
    auto load = [&](int s, u32x4 &xv, float (&av)[MT]) {
        const long long pix = p0 + 16LL * s + 4 * wave + q;
        const bool in = pix < pend;
        if constexpr (K == 1) {
            xv = wg_load_x(xs, (size_t)pix * p.Cx, in && chok, p.xvec);
        } else {
            // the tap's pixel p + d_t, zero where it leaves p's own image (row h + ddy, column w + ddx of the same n)
            const int row = (int)(pix / p.W), w = (int)(pix - (long long)row * p.W) + ddx, h = row % p.H + ddy;
            const bool inside = (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
            xv = wg_load_x(xs, (size_t)(pix + ddy * p.W + ddx) * p.Cx, in && chok && inside, p.xvec);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) av[m] = in && rowok[m] ? ds[(size_t)pix * p.Cy + 16 * m] : 0.f;
    };
#pragma unroll
    for (int u = 0; u < WG_RING; ++u) load(u, xr[u], ar[u]);   // (a step past the slab loads nothing: zeros)
    for (int s0 = 0; s0 < steps; s0 += WG_RING) {
#pragma unroll
        for (int u = 0; u < WG_RING; ++u) {
            const u32x4 xv = xr[u];
            float av[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) av[m] = ar[u][m];
            load(s0 + WG_RING + u, xr[u], ar[u]);
            float b[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                b[2 * k] = __uint_as_float(xv[k] << 16);
                b[2 * k + 1] = __uint_as_float(xv[k] & 0xffff0000u);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                dbacc[m] += av[m];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], b[j], acc[m][j], 0, 0, 0);
            }
        }
    }

    // db: the four pixel quarters of a wave ((q0 + q1) + (q2 + q3), the same in every lane), then the waves in order
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        dbacc[m] += __shfl_xor(dbacc[m], 16, 64);
        dbacc[m] += __shfl_xor(dbacc[m], 32, 64);
        if (q == 0) s_db[wave][16 * m + c] = dbacc[m];
    }
    // dw: waves 1, 2, 3 hand their accumulators to wave 0 one after the other: ((a0 + a1) + a2) + a3
    for (int r = 1; r < 4; ++r) {
        if (wave == r) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s_acc[((m * 8 + j) * 4 + e) * 64 + lane] = acc[m][j][e];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[m][j][e] += s_acc[((m * 8 + j) * 4 + e) * 64 + lane];
        }
        __syncthreads();
    }
    if (blockIdx.y == 0 && threadIdx.x < 16 * MT) {
        const int t = threadIdx.x, o = ob + t;
        const float v = ((s_db[0][t] + s_db[1][t]) + s_db[2][t]) + s_db[3][t];
        if (o < p.R) ws_db[(size_t)slab * p.R + o] = v;
    }
    if (wave == 0 && chok) {
        // accumulator element e of tile (m, j): row 16 m + 4 q + e, channel ch + j: eight consecutive floats per row and lane
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = ob + 16 * m + 4 * q + e;
                if (o < p.R) {
                    float *dst = ws_dw + ((size_t)slab * p.R + o) * ncol + ch;
                    *(f32x4 *)dst = (f32x4){acc[m][0][e], acc[m][1][e], acc[m][2][e], acc[m][3][e]};
                    *(f32x4 *)(dst + 4) = (f32x4){acc[m][4][e], acc[m][5][e], acc[m][6][e], acc[m][7][e]};
                }
            }
    }
}

template <int MT, int K>
__global__ __launch_bounds__(256) void conv1x1_wgrad_kernel(const uint16_t *__restrict__ x, const float *__restrict__ dy, WgParams p,
                                                            float *__restrict__ ws_dw, float *__restrict__ ws_db) {
    wgrad_body<MT, K>(x, dy, p, ws_dw, ws_db, blockIdx.z * 16 * MT);
}

// md_conv2d_grouped_bwd_weight: the same body, blockIdx.z is the group; its channel offsets, its cout and its part of the workspace come
// from the table (one 16-row tile per group: cout <= 16)
struct GroupTable {
    int G, per_dw, per_db;   // floats of one group's dw / db partials in the workspace
    int cout[MD_GROUPED_MAX_GROUPS], y_off[MD_GROUPED_MAX_GROUPS], w_row[MD_GROUPED_MAX_GROUPS];
};

template <int K>
__global__ __launch_bounds__(256) void grouped_wgrad_kernel(const uint16_t *__restrict__ x, const float *__restrict__ dy, WgParams p, GroupTable t,
                                                            float *__restrict__ ws_dw, float *__restrict__ ws_db) {
    const int g = blockIdx.z;
    p.x_c_off += 64 * g;
    p.dy_c_off = t.y_off[g];
    p.cout = t.cout[g];
    wgrad_body<1, K>(x, dy, p, ws_dw + (size_t)g * t.per_dw, ws_db + (size_t)g * t.per_db, 0);
}

// the sum of one element's slab partials: WG_WAYS interleaved chains over the slabs, then the chains in order
__device__ __forceinline__ float wgrad_sum_slabs(const float *__restrict__ src, size_t stride, int n_slabs, float (&red)[WG_WAYS][32], int t, int way) {
    float acc = 0.f;
    if (src) {
#pragma unroll 4
        for (int s = way; s < n_slabs; s += WG_WAYS) acc += src[(size_t)s * stride];
    }
    red[way][t] = acc;
    __syncthreads();
    float v = red[0][t];
#pragma unroll
    for (int k = 1; k < WG_WAYS; ++k) v += red[k][t];
    return src ? v + 0.f : 0.f;   // (a sum of -0.0 alone leaves +0.0 as well)
}

// one element of dw (flat index < rows kpad) or db (behind them) per lane & 31; lane >> 5 is the chain
// G (md_conv_bwd_weight beyond kernel 1 / korder 0 / dense): the element's column is col(t, i) of the header, and an (o, i) outside the
// blocks has no source: +0.0
template <bool G>
__global__ __launch_bounds__(256) void conv1x1_wgrad_sum_kernel(const float *__restrict__ ws_dw, const float *__restrict__ ws_db, WgParams p,
                                                                float *__restrict__ dw, float *__restrict__ db) {
    __shared__ float red[WG_WAYS][32];
    const int t = threadIdx.x & 31, way = threadIdx.x >> 5;
    const long long n_dw = (long long)p.rows * p.kpad, total = n_dw + p.rowsb;
    const long long e = (long long)blockIdx.x * 32 + t;
    const float *src = nullptr;
    size_t stride = 0;
    if (e < n_dw) {
        const int o = (int)(e / p.kpad), i = (int)(e - (long long)o * p.kpad);
        if constexpr (!G) {
            if (o < p.cout && i < p.cin) {
                src = ws_dw + (size_t)o * p.cin + i;
                stride = (size_t)p.R * p.cin;
            }
        } else if (o < p.cout && i < p.KK) {
            int t, ci;   // column i of dw is tap t, channel ci
            if (p.korder) {
                const int g = i / (p.taps * 64), r = i - g * (p.taps * 64);
                t = r >> 6;
                ci = g * 64 + (r & 63);
            } else {
                t = i / p.cin;
                ci = i - t * p.cin;
            }
            bool live = p.n_blocks == 0;
            for (int b = 0; b < p.n_blocks; ++b)
                live = live || (o >= p.blk[b].row0 && o < p.blk[b].row0 + p.blk[b].rows && ci >= p.blk[b].col0 && ci < p.blk[b].col0 + p.blk[b].cols);
            if (live) {
                src = ws_dw + (size_t)o * p.KK + t * p.cin + ci;
                stride = (size_t)p.R * p.KK;
            }
        }
    } else if (e < total) {
        const int o = (int)(e - n_dw);
        if (o < p.cout) {
            src = ws_db + o;
            stride = (size_t)p.R;
        }
    }
    const float v = wgrad_sum_slabs(src, stride, p.n_slabs, red, t, way);
    if (way == 0 && e < total) {
        if (e < n_dw) dw[e] = v;
        else db[e - n_dw] = v;
    }
}

// md_conv2d_grouped_bwd_weight: an element of dw[R][KK] / db[R] belongs to the group whose rows hold it (none: +0.0)
__global__ __launch_bounds__(256) void grouped_wgrad_sum_kernel(const float *__restrict__ ws_dw, const float *__restrict__ ws_db, WgParams p, GroupTable tb,
                                                                float *__restrict__ dw, float *__restrict__ db) {
    __shared__ float red[WG_WAYS][32];
    const int t = threadIdx.x & 31, way = threadIdx.x >> 5;
    const long long n_dw = (long long)p.rows * p.kpad, total = n_dw + p.rowsb;
    const long long e = (long long)blockIdx.x * 32 + t;
    const float *src = nullptr;
    size_t stride = 0;
    if (e < total) {
        const bool is_w = e < n_dw;
        const int o = is_w ? (int)(e / p.kpad) : (int)(e - n_dw), i = is_w ? (int)(e - (long long)o * p.kpad) : 0;
        for (int g = 0; g < tb.G; ++g) {
            const int r = o - tb.w_row[g];
            if (r >= 0 && r < tb.cout[g]) {
                src = is_w ? ws_dw + (size_t)g * tb.per_dw + (size_t)r * p.KK + i : ws_db + (size_t)g * tb.per_db + r;
                stride = is_w ? (size_t)p.R * p.KK : (size_t)p.R;
            }
        }
    }
    const float v = wgrad_sum_slabs(src, stride, p.n_slabs, red, t, way);
    if (way == 0 && e < total) {
        if (e < n_dw) dw[e] = v;
        else db[e - n_dw] = v;
    }
}

// scratch of md_conv1x1_bwd_weight: dw partials [n_slabs][R][cin] f32 at 0, then db partials [n_slabs][R] f32
struct WgScratch { int64_t S, n_slabs, R, db, total; };
static WgScratch wgrad_scratch(Sz P, Sz cin, Sz cout) {
    const Sz per = (P + (MD_CONV1X1_BWD_MAX_SLABS - 1)) / MD_CONV1X1_BWD_MAX_SLABS;
    Sz S = (per + 15) / 16 * 16;
    if (S < MD_CONV1X1_BWD_SLAB_MIN) S = MD_CONV1X1_BWD_SLAB_MIN;
    const Sz n_slabs = (P + S - 1) / S, R = (cout + 15) / 16 * 16, db = 4 * n_slabs * R * cin, total = db + 4 * n_slabs * R;
    return {(int64_t)S, (int64_t)n_slabs, (int64_t)R, (int64_t)db, (int64_t)total};
}

template <int K>
static void wgrad_launch(int mt, dim3 grid, hipStream_t s, const uint16_t *x, const float *dy, const WgParams &p, float *ws_dw, float *ws_db) {
    if (mt == 1) hipLaunchKernelGGL((conv1x1_wgrad_kernel<1, K>), grid, dim3(256), 0, s, x, dy, p, ws_dw, ws_db);
    else if (mt == 2) hipLaunchKernelGGL((conv1x1_wgrad_kernel<2, K>), grid, dim3(256), 0, s, x, dy, p, ws_dw, ws_db);
    else hipLaunchKernelGGL((conv1x1_wgrad_kernel<4, K>), grid, dim3(256), 0, s, x, dy, p, ws_dw, ws_db);
}

// md_conv1x1_bwd_weight (kxk false: md_conv1x1_bwd_attrs, a kernel-1, korder-0, dense layer) and md_conv_bwd_weight (md_conv_bwd_attrs)
static int conv_bwd_weight_entry(MD_AOT_ARGS, bool kxk) {
    // in : x[N,H,W,Cx] bf16, dy[N,H,W,Cy] f32 ; out: dw[rows,kpad] f32, db[rowsb] f32 or NULL ; [workspace]
    const int WS = 4;
    Args a(MD_ARGS, WS, WS + 1);
    md_conv_bwd_attrs full;
    memset(&full, 0, sizeof(full));
    full.kernel = 1;
    if (kxk) {
        const md_conv_bwd_attrs *at = a.attrs<md_conv_bwd_attrs>(extra);
        if (at) full = *at;
    } else {
        const md_conv1x1_bwd_attrs *at = a.attrs<md_conv1x1_bwd_attrs>(extra);
        if (at) { full.cin = at->cin; full.cout = at->cout; full.x_c_off = at->x_c_off; full.dy_c_off = at->dy_c_off; full.reserved0 = at->reserved0; }
    }
    const md_conv_bwd_attrs *at = &full;
    a.tensor(0, BF16, 4); a.tensor(1, F32, 4); a.tensor(2, F32, 2); a.optional(3, F32, 1);
    a.scratch(WS);
    if (int rc = a.rc()) return rc;
    const int64_t N = a.d(0, 0), H = a.d(0, 1), W = a.d(0, 2), Cx = a.d(0, 3), Cy = a.d(1, 3);
    const bool with_db = a.given(3);
    a.require(N >= 1 && H >= 1 && W >= 1 && Cx >= 1 && Cy >= 1);
    a.require(a.d(1, 0) == N && a.d(1, 1) == H && a.d(1, 2) == W);
    a.require(at->reserved0 == 0 && at->cin >= 1 && at->cout >= 1 && at->x_c_off >= 0 && at->dy_c_off >= 0);
    a.require((at->kernel == 1 || at->kernel == 3) && (at->korder == 0 || at->korder == 1) && at->n_blocks >= 0 && at->n_blocks <= MD_CONV_BWD_MAX_BLOCKS);
    if (int rc = a.rc()) return rc;
    const int64_t cin = at->cin, cout = at->cout, taps = at->kernel * at->kernel, KK = taps * cin;
    for (int b = 0; b < at->n_blocks; ++b) {
        const md_conv_bwd_block &k = at->blocks[b];
        a.require(k.row0 >= 0 && k.rows >= 1 && k.col0 >= 0 && k.cols >= 1 && (int64_t)k.row0 + k.rows <= cout && (int64_t)k.col0 + k.cols <= cin);
    }
    a.require(at->x_c_off + cin <= Cx && at->dy_c_off + cout <= Cy);
    a.require(a.d(2, 0) >= cout && a.d(2, 1) >= KK && (!with_db || a.d(3, 0) >= cout));
    a.require(!aliased(params, 2, 4));
    if (int rc = a.rc()) return rc;
    const int64_t lim = (int64_t)1 << 31;
    if (cin % 8 != 0 || cin > (at->kernel == 1 ? MD_CONV_BWD_MAX_CIN_K1 : MD_CONV_BWD_MAX_CIN_K3) || cout > MD_CONV_BWD_MAX_COUT) return MD_ERR_SIZE;
    if (at->korder == 1 && cin % 64 != 0) return MD_ERR_SIZE;
    if (N >= lim || H >= lim || W >= lim || mul({N, H}) >= lim || mul({N, H, W}) >= lim) return MD_ERR_SIZE;
    const int64_t P = mul({N, H, W});
    if (add(a.numel(2), with_db ? a.numel(3) : 0) >= lim) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2})) return MD_ERR_ARG;
    const WgScratch w = wgrad_scratch(P, KK, cout);
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = acquire_aligned(ws, (size_t)w.total, a, WS, s, 16)) return rc;

    WgParams p;
    memset(&p, 0, sizeof(p));
    p.P = (int)P; p.S = (int)w.S; p.n_slabs = (int)w.n_slabs; p.cin = (int)cin; p.cout = (int)cout; p.R = (int)w.R;
    p.Cx = (int)Cx; p.Cy = (int)Cy; p.x_c_off = at->x_c_off; p.dy_c_off = at->dy_c_off;
    p.xvec = Cx % 8 == 0 && at->x_c_off % 8 == 0 && (uintptr_t)params[0] % 16 == 0;
    p.rows = (int)a.d(2, 0); p.kpad = (int)a.d(2, 1); p.rowsb = with_db ? (int)a.d(3, 0) : 0;
    p.KK = (int)KK; p.taps = (int)taps; p.H = (int)H; p.W = (int)W; p.korder = at->korder; p.n_blocks = at->n_blocks;
    for (int b = 0; b < at->n_blocks; ++b) p.blk[b] = at->blocks[b];
    const uint16_t *x = (const uint16_t *)params[0];
    const float *dy = (const float *)params[1];
    float *ws_dw = (float *)ws.ptr, *ws_db = (float *)((char *)ws.ptr + w.db);
    const int mt = cout <= 16 ? 1 : (cout <= 32 ? 2 : 4);
    const dim3 grid((unsigned)w.n_slabs, (unsigned)((KK + WG_GROUP - 1) / WG_GROUP), (unsigned)((cout + 16 * mt - 1) / (16 * mt)));
    if (at->kernel == 1) wgrad_launch<1>(mt, grid, s, x, dy, p, ws_dw, ws_db);
    else wgrad_launch<3>(mt, grid, s, x, dy, p, ws_dw, ws_db);
    const int64_t elems = (int64_t)p.rows * p.kpad + p.rowsb;
    const dim3 sgrid((unsigned)((elems + 31) / 32));
    float *dw = (float *)params[2], *db = with_db ? (float *)params[3] : nullptr;
    if (at->kernel == 1 && at->korder == 0 && at->n_blocks == 0) hipLaunchKernelGGL(conv1x1_wgrad_sum_kernel<false>, sgrid, dim3(256), 0, s, ws_dw, ws_db, p, dw, db);
    else hipLaunchKernelGGL(conv1x1_wgrad_sum_kernel<true>, sgrid, dim3(256), 0, s, ws_dw, ws_db, p, dw, db);
    return launched();
}

// ---------------------------------------------------------------------------------------------------- md_conv1x1_bwd_data
constexpr int DG_PIXELS = 256;   // pixels per workgroup: four steps of 16 per wave behind one fill of the weight tile

struct DgParams {
    int P, cin, cout, kq;                        // kq: o-quads of the reduction, ceil(cout / 4)
    int Cy, Cdx, Ca, kpad, dy_c_off, dx_c_off, act_c_off;
    int wvec, avec, dxvec, has_act;              // 16-byte paths: every chunk of w / act / dx the layer touches is aligned
};

__global__ __launch_bounds__(256) void conv1x1_dgrad_kernel(const float *__restrict__ dy, const uint16_t *__restrict__ w,
                                                            const uint16_t *__restrict__ act, DgParams p, float *__restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) uint16_t s_w[];   // [4 kq][128]: w[o][128 g + ..], zero past cout and past cin
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int g0 = blockIdx.y * WG_GROUP, ch = g0 + 8 * c;
    const bool chok = ch < p.cin;
    for (int k = threadIdx.x; k < 4 * p.kq * 16; k += 256) {
        const int o = k >> 4, cc = g0 + 8 * (k & 15);
        *(u32x4 *)(s_w + (size_t)k * 8) = wg_load_x(w, (size_t)o * p.kpad + cc, o < p.cout && cc < p.cin, p.wvec);
    }
    __syncthreads();

    const float *ds = dy + p.dy_c_off + q;
    for (int step = 0; step < DG_PIXELS / 64; ++step) {
        const long long base = (long long)blockIdx.x * DG_PIXELS + 64 * step + 16 * wave;
        if (base >= p.P) break;
        const long long pa = base + c;                          // the MFMA row this lane feeds
        const bool rowok = pa < p.P;
        const float *dp = ds + (size_t)(rowok ? pa : 0) * p.Cy;
        f32x4 acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < p.kq; ++s) {
            const float av = rowok && 4 * s + q < p.cout ? dp[4 * s] : 0.f;
            const u32x4 wv = *(const u32x4 *)(s_w + ((size_t)(4 * s + q) * 16 + c) * 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[2 * k] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __uint_as_float(wv[k] << 16), acc[2 * k], 0, 0, 0);
                acc[2 * k + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, __uint_as_float(wv[k] & 0xffff0000u), acc[2 * k + 1], 0, 0, 0);
            }
        }
        // accumulator element e of tile j: pixel base + 4 q + e, channel ch + j: eight consecutive floats per pixel and lane
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long pix = base + 4 * q + e;
            if (!chok || pix >= p.P) continue;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = acc[j][e];
            if (p.has_act) {
                const u32x4 m = wg_load_x(act, (size_t)pix * p.Ca + p.act_c_off + ch, true, p.avec);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[2 * k] = __uint_as_float(m[k] << 16) > 0.f ? v[2 * k] : 0.f;               // (false for -0, a negative, a NaN)
                    v[2 * k + 1] = __uint_as_float(m[k] & 0xffff0000u) > 0.f ? v[2 * k + 1] : 0.f;
                }
            }
            float *dst = dx + (size_t)pix * p.Cdx + p.dx_c_off + ch;
            if (p.dxvec) {
                *(f32x4 *)dst = (f32x4){v[0], v[1], v[2], v[3]};
                *(f32x4 *)(dst + 4) = (f32x4){v[4], v[5], v[6], v[7]};
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) dst[j] = v[j];
            }
        }
    }
}

static int conv1x1_bwd_data_entry(MD_AOT_ARGS) {
    // in : dy[N,H,W,Cy] f32, w[rows,kpad] bf16, act[N,H,W,Ca] bf16 or NULL ; out: dx[N,H,W,Cdx] f32
    Args a(MD_ARGS, 4, 4);
    const md_conv1x1_bwd_data_attrs *at = a.attrs<md_conv1x1_bwd_data_attrs>(extra);
    a.tensor(0, F32, 4); a.tensor(1, BF16, 2); a.optional(2, BF16, 4); a.tensor(3, F32, 4);
    if (int rc = a.rc()) return rc;
    const int64_t N = a.d(0, 0), H = a.d(0, 1), W = a.d(0, 2), Cy = a.d(0, 3), Cdx = a.d(3, 3);
    const bool with_act = a.given(2);
    const int64_t Ca = with_act ? a.d(2, 3) : 0;
    a.require(N >= 1 && H >= 1 && W >= 1 && Cy >= 1 && Cdx >= 1);
    a.require(a.d(3, 0) == N && a.d(3, 1) == H && a.d(3, 2) == W);
    a.require(!with_act || (a.d(2, 0) == N && a.d(2, 1) == H && a.d(2, 2) == W && Ca >= 1));
    a.require(at->reserved0 == 0 && at->cin >= 1 && at->cout >= 1 && at->dy_c_off >= 0 && at->dx_c_off >= 0 && at->act_c_off >= 0);
    if (int rc = a.rc()) return rc;
    const int64_t cin = at->cin, cout = at->cout;
    a.require(at->dy_c_off + cout <= Cy && at->dx_c_off + cin <= Cdx && (with_act ? at->act_c_off + cin <= Ca : at->act_c_off == 0));
    a.require(a.d(1, 0) >= cout && a.d(1, 1) >= cin);
    a.require(!aliased(params, 3, 4));
    if (int rc = a.rc()) return rc;
    const int64_t lim = (int64_t)1 << 31;
    if (cin % 8 != 0 || cin > MD_CONV1X1_BWD_DATA_MAX_CIN || cout > MD_CONV1X1_BWD_DATA_MAX_COUT) return MD_ERR_SIZE;
    if (N >= lim || H >= lim || W >= lim || mul({N, H}) >= lim || mul({N, H, W}) >= lim) return MD_ERR_SIZE;
    const int64_t P = mul({N, H, W});
    if (mul({P, Cy}) >= lim || mul({P, Cdx}) >= lim || mul({P, Ca}) >= lim || a.numel(1) >= lim) return MD_ERR_SIZE;
    if (!a.have({0, 1, 3})) return MD_ERR_ARG;

    DgParams p;
    memset(&p, 0, sizeof(p));
    p.P = (int)P; p.cin = (int)cin; p.cout = (int)cout; p.kq = (int)((cout + 3) / 4);
    p.Cy = (int)Cy; p.Cdx = (int)Cdx; p.Ca = (int)Ca; p.kpad = (int)a.d(1, 1);
    p.dy_c_off = at->dy_c_off; p.dx_c_off = at->dx_c_off; p.act_c_off = at->act_c_off; p.has_act = with_act;
    p.wvec = p.kpad % 8 == 0 && (uintptr_t)params[1] % 16 == 0;
    p.avec = with_act && Ca % 8 == 0 && at->act_c_off % 8 == 0 && (uintptr_t)params[2] % 16 == 0;
    p.dxvec = Cdx % 4 == 0 && at->dx_c_off % 4 == 0 && (uintptr_t)params[3] % 16 == 0;
    const dim3 grid((unsigned)((P + DG_PIXELS - 1) / DG_PIXELS), (unsigned)((cin + WG_GROUP - 1) / WG_GROUP));
    const size_t lds = (size_t)4 * p.kq * WG_GROUP * sizeof(uint16_t);   // at most 256 x 128 x 2 = 64 KiB
    hipLaunchKernelGGL(conv1x1_dgrad_kernel, grid, dim3(256), lds, (hipStream_t)stream, (const float *)params[0], (const uint16_t *)params[1],
                       with_act ? (const uint16_t *)params[2] : nullptr, p, (float *)params[3]);
    return launched();
}

// ---------------------------------------------------------------------------------------------------- md_conv2d_grouped_bwd_*
// the forward table as both backward operators take it: R rows of the pack, Cy channels of dy, Cs channels of the tensor(s) the groups'
// 64-channel slices lie in (x; dx and act).  Every check of the table; the caller asks a.rc() behind it.
static void grouped_table_checks(Args &a, const md_conv2d_grouped_attrs *at, int64_t R, int64_t Cy, int64_t Cs, bool disjoint_rows) {
    if (!a.require(at->reserved0 == 0 && (at->k == 1 || at->k == 3) && at->relu == 0 && at->cin_g == 64)) return;
    if (!a.require(at->groups >= 1 && at->groups <= MD_GROUPED_MAX_GROUPS)) return;
    a.require(at->x_c_off >= 0 && at->x_c_off + (int64_t)at->groups * 64 <= Cs);
    for (int g = 0; g < at->groups; ++g) {
        const int64_t co = at->cout[g], yo = at->y_off[g], wr = at->w_row[g];
        a.require(co >= 1 && co <= 16 && yo >= 0 && yo + co <= Cy && wr >= 0 && wr + co <= R);
        for (int h = 0; disjoint_rows && h < g; ++h)   // two groups summing into one row of dw
            a.require(!(wr < (int64_t)at->w_row[h] + at->cout[h] && at->w_row[h] < wr + co));
    }
}

// 16-pixel steps of a wave behind one read of a w fragment.  One: the kernel waits on its dy and act loads, so waves per SIMD count
// (83 VGPRs); four steps (232 VGPRs, two waves per SIMD) took 1.56x the time at the nuScenes shape
constexpr int GD_STEPS = MD_GROUPED_BWD_TILE / 64;

struct GdParams {
    int P, H, W, Cy, Cdx, Ca, KW;             // KW = k k 64, a row of the pack
    int x_c_off, has_act, wvec, avec, dxvec;  // wide paths: every 8-byte piece of w / act and every 16-byte piece of dx is aligned
    int G;
    int cout[MD_GROUPED_MAX_GROUPS], y_off[MD_GROUPED_MAX_GROUPS], w_row[MD_GROUPED_MAX_GROUPS];
};

// grid (ceil(P / MD_GROUPED_BWD_TILE), ceil(G / MD_GROUPED_BWD_WALK)).  Lane (c, q) feeds MFMA row c (pixel c of a step) with
// dy[pixel - d_t][o = 4 s + q] and column c of MFMA j with w[o][t 64 + 4 c + j]: after the four MFMAs of a step the lane holds channels
// 4 c .. 4 c + 3 of pixels 4 q .. 4 q + 3 and stores each as one 16-byte row, 256 contiguous bytes per pixel and group.  The taps are
// unrolled, so a group's nine dy loads per lane are in flight together.
template <int K>
__global__ __launch_bounds__(256, 4) void grouped_dgrad_kernel(const float *__restrict__ dy, const uint16_t *__restrict__ w,
                                                            const uint16_t *__restrict__ act, GdParams p, float *__restrict__ dx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const long long base = (long long)blockIdx.x * MD_GROUPED_BWD_TILE + 16 * GD_STEPS * wave;
    if (base >= p.P) return;   // the whole wave; the kernel has no barrier
    long long pix[GD_STEPS];   // the pixel of the MFMA row this lane feeds in step u, its row and column in its own image
    int ph[GD_STEPS], pw[GD_STEPS];
#pragma unroll
    for (int u = 0; u < GD_STEPS; ++u) {
        pix[u] = base + 16 * u + c;
        const long long pc = pix[u] < p.P ? pix[u] : 0;
        const int row = (int)(pc / p.W);
        pw[u] = (int)(pc - (long long)row * p.W);
        ph[u] = row % p.H;
    }
    for (int gi = 0; gi < MD_GROUPED_BWD_WALK; ++gi) {
        const int g = blockIdx.y * MD_GROUPED_BWD_WALK + gi;
        if (g >= p.G) break;
        const int cout = p.cout[g], cq = (cout + 3) >> 2;
        const float *dg = dy + p.y_off[g];
        const uint16_t *wg = w + (size_t)p.w_row[g] * p.KW + 4 * c;
        f32x4 acc[GD_STEPS][4];
#pragma unroll
        for (int u = 0; u < GD_STEPS; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[u][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < K * K; ++t) {
            const int ddy = t / K - K / 2, ddx = t % K - K / 2;
            // the term's pixel q - d_t, inside q's own image or no term
            bool in[GD_STEPS];
            size_t off[GD_STEPS];
#pragma unroll
            for (int u = 0; u < GD_STEPS; ++u) {
                in[u] = pix[u] < p.P && (unsigned)(ph[u] - ddy) < (unsigned)p.H && (unsigned)(pw[u] - ddx) < (unsigned)p.W;
                off[u] = in[u] ? (size_t)(pix[u] - ddy * p.W - ddx) * p.Cy : 0;
            }
            for (int s = 0; s < cq; ++s) {
                const int o = 4 * s + q;
                const bool live = o < cout;
                unsigned w01 = 0u, w23 = 0u;   // w[o][t 64 + 4 c .. + 3]; rows past cout are zero
                if (live) {
                    const uint16_t *wp = wg + (size_t)o * p.KW + t * 64;
                    if (p.wvec) {
                        const u32x2 v = *(const u32x2 *)wp;
                        w01 = v[0];
                        w23 = v[1];
                    } else {
                        w01 = (unsigned)wp[0] | ((unsigned)wp[1] << 16);
                        w23 = (unsigned)wp[2] | ((unsigned)wp[3] << 16);
                    }
                }
                const float b0 = __uint_as_float(w01 << 16), b1 = __uint_as_float(w01 & 0xffff0000u);
                const float b2 = __uint_as_float(w23 << 16), b3 = __uint_as_float(w23 & 0xffff0000u);
#pragma unroll
                for (int u = 0; u < GD_STEPS; ++u) {
                    const float av = in[u] && live ? dg[off[u] + o] : 0.f;
                    acc[u][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc[u][0], 0, 0, 0);
                    acc[u][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc[u][1], 0, 0, 0);
                    acc[u][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b2, acc[u][2], 0, 0, 0);
                    acc[u][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b3, acc[u][3], 0, 0, 0);
                }
            }
        }
        // accumulator element e of MFMA j in step u: pixel base + 16 u + 4 q + e, channel 64 g + 4 c + j
        const int chn = p.x_c_off + 64 * g + 4 * c;
#pragma unroll
        for (int u = 0; u < GD_STEPS; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long px = base + 16 * u + 4 * q + e;
                if (px >= p.P) continue;
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = acc[u][j][e];
                if (p.has_act) {
                    const uint16_t *ap = act + (size_t)px * p.Ca + chn;
                    unsigned m01, m23;
                    if (p.avec) {
                        const u32x2 m = *(const u32x2 *)ap;
                        m01 = m[0];
                        m23 = m[1];
                    } else {
                        m01 = (unsigned)ap[0] | ((unsigned)ap[1] << 16);
                        m23 = (unsigned)ap[2] | ((unsigned)ap[3] << 16);
                    }
                    v[0] = __uint_as_float(m01 << 16) > 0.f ? v[0] : 0.f;            // (false for -0, a negative, a NaN)
                    v[1] = __uint_as_float(m01 & 0xffff0000u) > 0.f ? v[1] : 0.f;
                    v[2] = __uint_as_float(m23 << 16) > 0.f ? v[2] : 0.f;
                    v[3] = __uint_as_float(m23 & 0xffff0000u) > 0.f ? v[3] : 0.f;
                }
                float *dst = dx + (size_t)px * p.Cdx + chn;
                if (p.dxvec) {
                    *(f32x4 *)dst = (f32x4){v[0], v[1], v[2], v[3]};
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) dst[j] = v[j];
                }
            }
    }
}

static int grouped_bwd_data_entry(MD_AOT_ARGS) {
    // in : dy[N,H,W,Cy] f32, w[R, k k 64] bf16, act[N,H,W,Ca] bf16 or NULL ; out: dx[N,H,W,Cdx] f32
    Args a(MD_ARGS, 4, 4);
    const md_conv2d_grouped_attrs *at = a.attrs<md_conv2d_grouped_attrs>(extra);
    a.tensor(0, F32, 4); a.tensor(1, BF16, 2); a.optional(2, BF16, 4); a.tensor(3, F32, 4);
    if (int rc = a.rc()) return rc;
    const int64_t N = a.d(0, 0), H = a.d(0, 1), W = a.d(0, 2), Cy = a.d(0, 3), Cdx = a.d(3, 3), R = a.d(1, 0);
    const bool with_act = a.given(2);
    const int64_t Ca = with_act ? a.d(2, 3) : 0;
    a.require(N >= 1 && H >= 1 && W >= 1 && Cy >= 1 && Cdx >= 1 && R >= 1);
    a.require(a.d(3, 0) == N && a.d(3, 1) == H && a.d(3, 2) == W);
    a.require(!with_act || (a.d(2, 0) == N && a.d(2, 1) == H && a.d(2, 2) == W));
    grouped_table_checks(a, at, R, Cy, with_act && Ca < Cdx ? Ca : Cdx, false);
    if (int rc = a.rc()) return rc;
    a.require(a.d(1, 1) == (int64_t)at->k * at->k * 64);
    a.require(!aliased(params, 3, 4));
    if (int rc = a.rc()) return rc;
    const int64_t lim = (int64_t)1 << 31;
    if (N >= lim || H >= lim || W >= lim || mul({N, H}) >= lim || mul({N, H, W}) >= lim) return MD_ERR_SIZE;
    const int64_t P = mul({N, H, W});
    if (mul({P, Cy}) >= lim || mul({P, Cdx}) >= lim || mul({P, Ca}) >= lim || a.numel(1) >= lim) return MD_ERR_SIZE;
    if (!a.have({0, 1, 3})) return MD_ERR_ARG;

    GdParams p;
    memset(&p, 0, sizeof(p));
    p.P = (int)P; p.H = (int)H; p.W = (int)W; p.Cy = (int)Cy; p.Cdx = (int)Cdx; p.Ca = (int)Ca; p.KW = at->k * at->k * 64;
    p.x_c_off = at->x_c_off; p.has_act = with_act; p.G = at->groups;
    p.wvec = (uintptr_t)params[1] % 8 == 0;
    p.avec = with_act && Ca % 4 == 0 && at->x_c_off % 4 == 0 && (uintptr_t)params[2] % 8 == 0;
    p.dxvec = Cdx % 4 == 0 && at->x_c_off % 4 == 0 && (uintptr_t)params[3] % 16 == 0;
    for (int g = 0; g < at->groups; ++g) { p.cout[g] = at->cout[g]; p.y_off[g] = at->y_off[g]; p.w_row[g] = at->w_row[g]; }
    const dim3 grid((unsigned)((P + MD_GROUPED_BWD_TILE - 1) / MD_GROUPED_BWD_TILE), (unsigned)((at->groups + MD_GROUPED_BWD_WALK - 1) / MD_GROUPED_BWD_WALK));
    const float *dy = (const float *)params[0];
    const uint16_t *w = (const uint16_t *)params[1], *act = with_act ? (const uint16_t *)params[2] : nullptr;
    if (at->k == 1) hipLaunchKernelGGL(grouped_dgrad_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, dy, w, act, p, (float *)params[3]);
    else hipLaunchKernelGGL(grouped_dgrad_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, dy, w, act, p, (float *)params[3]);
    return launched();
}

// scratch of md_conv2d_grouped_bwd_weight: per group the scratch of md_conv_bwd_weight for one group (cin 64, one 16-row tile), the groups'
// dw partials back to back at 0, then their db partials
struct GwScratch { WgScratch one; int64_t per_dw, per_db, db, total; };
static GwScratch grouped_wgrad_scratch(Sz P, Sz groups, Sz k) {
    GwScratch s;
    s.one = wgrad_scratch(P, k * k * 64, 16);
    const Sz db = s.one.db, total = s.one.total;      // (INT64_MAX where the one-group layout does not fit: it stays so below)
    s.per_dw = (int64_t)(db / 4);
    s.per_db = (int64_t)((total - db) / 4);
    s.db = (int64_t)(groups * db);
    s.total = (int64_t)(groups * total);
    return s;
}

static int grouped_bwd_weight_entry(MD_AOT_ARGS) {
    // in : x[N,H,W,C] bf16, dy[N,H,W,Cy] f32 ; out: dw[R, k k 64] f32, db[R] f32 or NULL ; [workspace]
    const int WS = 4;
    Args a(MD_ARGS, WS, WS + 1);
    const md_conv2d_grouped_attrs *at = a.attrs<md_conv2d_grouped_attrs>(extra);
    a.tensor(0, BF16, 4); a.tensor(1, F32, 4); a.tensor(2, F32, 2); a.optional(3, F32, 1);
    a.scratch(WS);
    if (int rc = a.rc()) return rc;
    const int64_t N = a.d(0, 0), H = a.d(0, 1), W = a.d(0, 2), Cx = a.d(0, 3), Cy = a.d(1, 3), R = a.d(2, 0);
    const bool with_db = a.given(3);
    a.require(N >= 1 && H >= 1 && W >= 1 && Cx >= 1 && Cy >= 1 && R >= 1);
    a.require(a.d(1, 0) == N && a.d(1, 1) == H && a.d(1, 2) == W);
    grouped_table_checks(a, at, R, Cy, Cx, true);
    if (int rc = a.rc()) return rc;
    const int64_t KK = (int64_t)at->k * at->k * 64, G = at->groups;
    a.require(a.d(2, 1) == KK && (!with_db || a.d(3, 0) == R));
    a.require(!aliased(params, 2, 4));
    if (int rc = a.rc()) return rc;
    const int64_t lim = (int64_t)1 << 31;
    if (N >= lim || H >= lim || W >= lim || mul({N, H}) >= lim || mul({N, H, W}) >= lim) return MD_ERR_SIZE;
    const int64_t P = mul({N, H, W});
    if (mul({P, Cx}) >= lim || mul({P, Cy}) >= lim || add(a.numel(2), with_db ? a.numel(3) : 0) >= lim) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2})) return MD_ERR_ARG;
    const GwScratch w = grouped_wgrad_scratch(P, G, at->k);
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = acquire_aligned(ws, (size_t)w.total, a, WS, s, 16)) return rc;

    WgParams p;   // one group's md_conv_bwd_weight call (cin 64, korder 0, dense); the kernel fills in the group's offsets and cout
    memset(&p, 0, sizeof(p));
    p.P = (int)P; p.S = (int)w.one.S; p.n_slabs = (int)w.one.n_slabs; p.cin = 64; p.cout = 0; p.R = (int)w.one.R;
    p.Cx = (int)Cx; p.Cy = (int)Cy; p.x_c_off = at->x_c_off; p.dy_c_off = 0;
    p.xvec = Cx % 8 == 0 && at->x_c_off % 8 == 0 && (uintptr_t)params[0] % 16 == 0;
    p.rows = (int)R; p.kpad = (int)KK; p.rowsb = with_db ? (int)R : 0;
    p.KK = (int)KK; p.taps = at->k * at->k; p.H = (int)H; p.W = (int)W;
    GroupTable t;
    memset(&t, 0, sizeof(t));
    t.G = (int)G; t.per_dw = (int)w.per_dw; t.per_db = (int)w.per_db;
    for (int g = 0; g < G; ++g) { t.cout[g] = at->cout[g]; t.y_off[g] = at->y_off[g]; t.w_row[g] = at->w_row[g]; }
    const uint16_t *x = (const uint16_t *)params[0];
    const float *dy = (const float *)params[1];
    float *ws_dw = (float *)ws.ptr, *ws_db = (float *)((char *)ws.ptr + w.db);
    const dim3 grid((unsigned)w.one.n_slabs, (unsigned)((KK + WG_GROUP - 1) / WG_GROUP), (unsigned)G);
    if (at->k == 1) hipLaunchKernelGGL(grouped_wgrad_kernel<1>, grid, dim3(256), 0, s, x, dy, p, t, ws_dw, ws_db);
    else hipLaunchKernelGGL(grouped_wgrad_kernel<3>, grid, dim3(256), 0, s, x, dy, p, t, ws_dw, ws_db);
    const int64_t elems = (int64_t)p.rows * p.kpad + p.rowsb;
    float *dw = (float *)params[2], *db = with_db ? (float *)params[3] : nullptr;
    hipLaunchKernelGGL(grouped_wgrad_sum_kernel, dim3((unsigned)((elems + 31) / 32)), dim3(256), 0, s, ws_dw, ws_db, p, t, dw, db);
    return launched();
}

}  // namespace md

using namespace md;

extern "C" int64_t md_conv1x1_bwd_weight_workspace_bytes(int64_t P, int64_t cin, int64_t cout) {
    return any_negative({P, cin, cout}) ? -1 : ws_answer(wgrad_scratch(P, cin, cout).total);
}
extern "C" int md_conv1x1_bwd_weight(MD_AOT_ARGS) { return conv_bwd_weight_entry(nparam, params, ndims, shapes, dtypes, stream, extra, false); }
extern "C" int64_t md_conv_bwd_weight_workspace_bytes(int64_t P, int64_t cin, int64_t cout, int64_t kernel) {
    if (any_negative({P, cin, cout}) || (kernel != 1 && kernel != 3)) return -1;
    return ws_answer(wgrad_scratch(P, Sz(kernel * kernel) * cin, cout).total);
}
extern "C" int md_conv_bwd_weight(MD_AOT_ARGS) { return conv_bwd_weight_entry(nparam, params, ndims, shapes, dtypes, stream, extra, true); }
extern "C" int md_conv1x1_bwd_data(MD_AOT_ARGS) { return conv1x1_bwd_data_entry(nparam, params, ndims, shapes, dtypes, stream, extra); }
extern "C" int md_conv2d_grouped_bwd_data(MD_AOT_ARGS) { return grouped_bwd_data_entry(nparam, params, ndims, shapes, dtypes, stream, extra); }
extern "C" int64_t md_conv2d_grouped_bwd_weight_workspace_bytes(int64_t P, int64_t groups, int64_t k) {
    return any_negative({P, groups}) || (k != 1 && k != 3) ? -1 : ws_answer(grouped_wgrad_scratch(P, groups, k).total);
}
extern "C" int md_conv2d_grouped_bwd_weight(MD_AOT_ARGS) { return grouped_bwd_weight_entry(nparam, params, ndims, shapes, dtypes, stream, extra); }

