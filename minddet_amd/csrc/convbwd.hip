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
#include <math.h>

#include "aot.h"
#include "device.h"
#include "../../include/minddet_hip_train.h"

#pragma clang fp contract(off)

namespace md {

static_assert(sizeof(md_conv1x1_bwd_attrs) == 5 * 4, "minddet_hip_train.h: attribute struct layout");

constexpr int WG_GROUP = 128;   // channels of x per workgroup column: 16 lanes x 8 bf16 = one 16-byte load per lane
constexpr int WG_RING = 4;      // pixel groups a wave loads ahead of its MFMAs
constexpr int WG_WAYS = MD_CONV1X1_BWD_SUM_WAYS;

struct WgParams {
    int P, S, n_slabs, cin, cout, R;      // R: rows of a partial block = cout rounded up to 16
    int Cx, Cy, x_c_off, dy_c_off, xvec;  // xvec: every 8-channel chunk of x the layer reads is 16-byte aligned
    int rows, kpad, rowsb;                // extents of dw and db (rowsb 0: no db)
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

template <int MT>
__global__ __launch_bounds__(256) void conv1x1_wgrad_kernel(const uint16_t *__restrict__ x, const float *__restrict__ dy, WgParams p,
                                                            float *__restrict__ ws_dw, float *__restrict__ ws_db) {
    __shared__ float s_acc[MT * 8 * 4 * 64];   // one wave's accumulators, [(m 8 + j) 4 + reg][lane]
    __shared__ float s_db[4][MT * 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, q = lane >> 4;
    const int slab = blockIdx.x, ch = blockIdx.y * WG_GROUP + 8 * c, ob = blockIdx.z * 16 * MT;
    const long long p0 = (long long)slab * p.S;
    const int pend = (int)min((long long)p.P, p0 + p.S);   // one past the slab's last pixel
    const bool chok = ch < p.cin;                          // (cin % 8 == 0: a chunk is inside the layer or outside it)
    bool rowok[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) rowok[m] = ob + 16 * m + c < p.cout;
    const uint16_t *xs = x + p.x_c_off + ch;
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
        xv = wg_load_x(xs, (size_t)pix * p.Cx, in && chok, p.xvec);
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
                    float *dst = ws_dw + ((size_t)slab * p.R + o) * p.cin + ch;
                    *(f32x4 *)dst = (f32x4){acc[m][0][e], acc[m][1][e], acc[m][2][e], acc[m][3][e]};
                    *(f32x4 *)(dst + 4) = (f32x4){acc[m][4][e], acc[m][5][e], acc[m][6][e], acc[m][7][e]};
                }
            }
    }
}

// one element of dw (flat index < rows kpad) or db (behind them) per lane & 31; lane >> 5 is the chain
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
        if (o < p.cout && i < p.cin) {
            src = ws_dw + (size_t)o * p.cin + i;
            stride = (size_t)p.R * p.cin;
        }
    } else if (e < total) {
        const int o = (int)(e - n_dw);
        if (o < p.cout) {
            src = ws_db + o;
            stride = (size_t)p.R;
        }
    }
    float acc = 0.f;
    if (src) {
#pragma unroll 4
        for (int s = way; s < p.n_slabs; s += WG_WAYS) acc += src[(size_t)s * stride];
    }
    red[way][t] = acc;
    __syncthreads();
    if (way == 0 && e < total) {
        float v = red[0][t];
#pragma unroll
        for (int k = 1; k < WG_WAYS; ++k) v += red[k][t];
        v = src ? v + 0.f : 0.f;   // (a sum of -0.0 alone leaves +0.0 as well)
        if (e < n_dw) dw[e] = v;
        else db[e - n_dw] = v;
    }
}

// scratch of md_conv1x1_bwd_weight: dw partials [n_slabs][R][cin] f32 at 0, then db partials [n_slabs][R] f32
struct WgScratch { int64_t S, n_slabs, R, db, total; };
static WgScratch wgrad_scratch(int64_t P, int64_t cin, int64_t cout) {
    WgScratch w;
    const int64_t per = (P + MD_CONV1X1_BWD_MAX_SLABS - 1) / MD_CONV1X1_BWD_MAX_SLABS;
    w.S = (per + 15) / 16 * 16;
    if (w.S < MD_CONV1X1_BWD_SLAB_MIN) w.S = MD_CONV1X1_BWD_SLAB_MIN;
    w.n_slabs = (P + w.S - 1) / w.S;
    w.R = (cout + 15) / 16 * 16;
    w.db = 4 * w.n_slabs * w.R * cin;
    w.total = w.db + 4 * w.n_slabs * w.R;
    return w;
}

static int conv1x1_bwd_weight_entry(MD_AOT_ARGS) {
    // in : x[N,H,W,Cx] bf16, dy[N,H,W,Cy] f32 ; out: dw[rows,kpad] f32, db[rowsb] f32 or NULL ; [workspace]
    const int WS = 4;
    Args a(MD_ARGS, WS, WS + 1);
    const md_conv1x1_bwd_attrs *at = a.attrs<md_conv1x1_bwd_attrs>(extra);
    a.tensor(0, BF16, 4); a.tensor(1, F32, 4); a.tensor(2, F32, 2); a.optional(3, F32, 1);
    a.optional(WS, U8);
    if (int rc = a.rc()) return rc;
    const int64_t N = a.d(0, 0), H = a.d(0, 1), W = a.d(0, 2), Cx = a.d(0, 3), Cy = a.d(1, 3);
    const bool with_db = a.given(3);
    a.require(N >= 1 && H >= 1 && W >= 1 && Cx >= 1 && Cy >= 1);
    a.require(a.d(1, 0) == N && a.d(1, 1) == H && a.d(1, 2) == W);
    a.require(at->reserved0 == 0 && at->cin >= 1 && at->cout >= 1 && at->x_c_off >= 0 && at->dy_c_off >= 0);
    if (int rc = a.rc()) return rc;
    const int64_t cin = at->cin, cout = at->cout;
    a.require(at->x_c_off + cin <= Cx && at->dy_c_off + cout <= Cy);
    a.require(a.d(2, 0) >= cout && a.d(2, 1) >= cin && (!with_db || a.d(3, 0) >= cout));
    a.require(!aliased(params, 2, 4));
    if (int rc = a.rc()) return rc;
    const int64_t lim = (int64_t)1 << 31;
    if (cin % 8 != 0 || cin > MD_CONV1X1_BWD_MAX_CIN || cout > MD_CONV1X1_BWD_MAX_COUT) return MD_ERR_SIZE;
    if (N >= lim || H >= lim || W >= lim || N * H >= lim || N * H * W >= lim) return MD_ERR_SIZE;
    const int64_t P = N * H * W;
    if (a.numel(2) + (with_db ? a.numel(3) : 0) >= lim) return MD_ERR_SIZE;
    if (!a.have({0, 1, 2})) return MD_ERR_ARG;
    const WgScratch w = wgrad_scratch(P, cin, cout);
    hipStream_t s = (hipStream_t)stream;
    Scratch ws;
    if (int rc = acquire_aligned(ws, (size_t)w.total, a, WS, s, 16)) return rc;

    WgParams p;
    memset(&p, 0, sizeof(p));
    p.P = (int)P; p.S = (int)w.S; p.n_slabs = (int)w.n_slabs; p.cin = (int)cin; p.cout = (int)cout; p.R = (int)w.R;
    p.Cx = (int)Cx; p.Cy = (int)Cy; p.x_c_off = at->x_c_off; p.dy_c_off = at->dy_c_off;
    p.xvec = Cx % 8 == 0 && at->x_c_off % 8 == 0 && (uintptr_t)params[0] % 16 == 0;
    p.rows = (int)a.d(2, 0); p.kpad = (int)a.d(2, 1); p.rowsb = with_db ? (int)a.d(3, 0) : 0;
    const uint16_t *x = (const uint16_t *)params[0];
    const float *dy = (const float *)params[1];
    float *ws_dw = (float *)ws.ptr, *ws_db = (float *)((char *)ws.ptr + w.db);
    const int mt = cout <= 16 ? 1 : (cout <= 32 ? 2 : 4);
    const dim3 grid((unsigned)w.n_slabs, (unsigned)((cin + WG_GROUP - 1) / WG_GROUP), (unsigned)((cout + 16 * mt - 1) / (16 * mt)));
    if (mt == 1) hipLaunchKernelGGL(conv1x1_wgrad_kernel<1>, grid, dim3(256), 0, s, x, dy, p, ws_dw, ws_db);
    else if (mt == 2) hipLaunchKernelGGL(conv1x1_wgrad_kernel<2>, grid, dim3(256), 0, s, x, dy, p, ws_dw, ws_db);
    else hipLaunchKernelGGL(conv1x1_wgrad_kernel<4>, grid, dim3(256), 0, s, x, dy, p, ws_dw, ws_db);
    const int64_t elems = (int64_t)p.rows * p.kpad + p.rowsb;
    hipLaunchKernelGGL(conv1x1_wgrad_sum_kernel, dim3((unsigned)((elems + 31) / 32)), dim3(256), 0, s, ws_dw, ws_db, p, (float *)params[2],
                       with_db ? (float *)params[3] : nullptr);
    return launched();
}

}  // namespace md

using namespace md;

extern "C" int64_t md_conv1x1_bwd_weight_workspace_bytes(int64_t P, int64_t cin, int64_t cout) {
    return any_negative({P, cin, cout}) ? -1 : wgrad_scratch(P, cin, cout).total;
}
extern "C" int md_conv1x1_bwd_weight(MD_AOT_ARGS) { return conv1x1_bwd_weight_entry(nparam, params, ndims, shapes, dtypes, stream, extra); }
