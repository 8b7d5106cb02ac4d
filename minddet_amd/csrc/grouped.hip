// grouped.hip -- a block-diagonal (grouped) convolution with many narrow groups in ONE launch: md_conv2d_grouped.
//
// What it replaces: the last conv of every SepHead branch of CenterPoint's CenterHead
// (minddet/models/centerpoint/det3d_ms/models/bbox_heads/center_head.py:28-99): 36 branches (6 tasks x reg 2, height 1, dim 3, rot 2,
// vel 2, hm 1 | 2), each a 3x3 conv 64 -> c with c in {1, 2, 3} on its own 64-channel slice of the 2304-channel intermediate that ONE
// md_conv2d writes for all 36 first convs.  As 36 md_conv2d launches each pads its 1-3 output channels to a 32-cout tile and re-plans a
// small grid; as one dense conv with a block-diagonal weight it would do 36x the MACs.
//
// Sizing (G = 36, N = 4, 128 x 128, derived from the shapes): the launch reads the 302 MB intermediate once and writes 9.4 MB, an HBM
// floor of ~39 us at 8 TB/s; the useful work is 5.3 GFLOP, the work at a 16-cout MFMA tile 43 GFLOP (~17 us at the 2.5 PF dense peak,
// ~36 us at the rate the ping-pong kernel sustains).  The tile choice: mfma_f32_16x16x32_bf16 with the group's couts as the 16 rows of A
// (rows >= cout_g are zero) and 16 pixels as the columns of B.  The 16-row padding costs MFMA time of the order of the HBM floor, which
// three resident workgroups per CU overlap with the tile loads; a VALU dot-product form would need the 64-channel operands per pixel and
// per tap in registers or LDS reads at 4 B per lane per MAC pair, LDS-bound well above this.
//
// A workgroup (4 waves) owns one group g and an 8 x 32 block of output pixels of one image:
//   load   the (8 + 2h) x (32 + 2h) halo tile of the group's 64 input channels into LDS (h = k / 2; zero outside the image), 16-B pieces,
//          the piece index XOR-swizzled with the pixel (p & 7) so that the 16 pixels of an MFMA column block read distinct banks
//   mma    each wave: 2 rows x 2 column blocks of 16 pixels, K = (tap, ci) in steps of 32 (18 steps at k = 3); the group's weights are
//          in registers for the whole tile (loaded once, rows >= cout_g zero)
//   store  lane l holds couts 4 (l >> 4) .. +3 of pixel l & 15: bias, ReLU, bf16, 2-B stores of the couts < cout_g
// Workgroup ids are XCD-swizzled so that consecutive work items -- the groups of one pixel tile, then the next tile -- run on the same
// XCD: their partial output lines merge in one L2 and the halo rows they share hit it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aot.h"
#include "device.h"

namespace md {

constexpr int GC_TH = 8, GC_TW = 32, GC_THREADS = 256;

struct GroupedArgs {
    const uint16_t *x;   // [N,H,W,C]
    const uint16_t *w;   // [R, k*k*64]
    const float *bias;   // [R]
    uint16_t *y;         // [N,H,W,Cy]
    int N, H, W, C, Cy, G;
    int x_c_off, relu;
    int tiles_x, tiles_y, n_work, work_per_xcd;
    int cout[MD_GROUPED_MAX_GROUPS], y_off[MD_GROUPED_MAX_GROUPS], w_row[MD_GROUPED_MAX_GROUPS];
};

template <int KS>
__global__ __launch_bounds__(GC_THREADS, 3) void grouped_conv_kernel(GroupedArgs a) {
    constexpr int HALO = KS / 2;
    constexpr int LH = GC_TH + 2 * HALO, LW = GC_TW + 2 * HALO;
    constexpr int PIECES = LH * LW * 8;                                 // 16-B pieces of the halo tile (64 channels = 8 pieces per pixel)
    constexpr int LOADS = (PIECES + GC_THREADS - 1) / GC_THREADS;
    constexpr int KSTEPS = KS * KS * 2;                                 // K = taps x 64, 32 per MFMA
    extern __shared__ __attribute__((aligned(16))) unsigned char gc_lds[];

    const int bid = blockIdx.x;
    const int work = (bid & 7) * a.work_per_xcd + (bid >> 3);           // consecutive work items on one XCD
    if (work >= a.n_work) return;                                       // whole workgroup, before any barrier
    const int g = work % a.G;
    const int tile = work / a.G;
    const int tx = tile % a.tiles_x, ty = (tile / a.tiles_x) % a.tiles_y, n = tile / (a.tiles_x * a.tiles_y);
    const int y0 = ty * GC_TH, x0 = tx * GC_TW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cout = a.cout[g];

    // ---- halo tile -> LDS (all loads issued before the first LDS write)
    const size_t img = (size_t)n * a.H * a.W;
    const int c0 = a.x_c_off + g * 64;
    u32x4 v[LOADS];
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
        const int p = tid + i * GC_THREADS;
        const int q = p >> 3, c = p & 7;
        const int yy = y0 - HALO + q / LW, xx = x0 - HALO + q % LW;
        v[i] = u32x4{0u, 0u, 0u, 0u};
        if (p < PIECES && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W)
            v[i] = *(const u32x4 *)(a.x + (img + (size_t)yy * a.W + xx) * a.C + c0 + c * 8);
    }
    // ---- the group's weights -> registers: lane l holds A[row l & 15][k = 32 s + 8 (l >> 4) .. +7], zero for rows >= cout
    constexpr int KW = KS * KS * 64;
    const int row = lane & 15, kq = lane >> 4;
    bf16x8 wf[KSTEPS];
    {
        const bool live = row < cout;
        const uint16_t *wr = a.w + (size_t)(a.w_row[g] + (live ? row : 0)) * KW + kq * 8;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            bf16x8 t = *(const bf16x8 *)(wr + s * 32);
            wf[s] = live ? t : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
        const int p = tid + i * GC_THREADS;
        if (p < PIECES) {
            const int q = p >> 3, c = p & 7;
            *(u32x4 *)(gc_lds + q * 128 + ((c ^ (q & 7)) << 4)) = v[i];
        }
    }
    __syncthreads();

    // ---- MFMA: wave w computes output rows 2w, 2w + 1, column blocks 0-15 and 16-31 of each
    f32x4 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        const int tap = s >> 1, ky = tap / KS, kx = tap % KS;
        const int piece = (s & 1) * 4 + kq;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int r = wave * 2 + (b >> 1), col = (b & 1) * 16 + row;
            const int q = (r + ky) * LW + col + kx;
            const bf16x8 bf = *(const bf16x8 *)(gc_lds + q * 128 + ((piece ^ (q & 7)) << 4));
            acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], bf, acc[b], 0, 0, 0);
        }
    }

    // ---- epilogue: lane l holds couts 4 kq .. +3 of pixel `row` of each column block
    float bs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = kq * 4 + j;
        bs[j] = c < cout ? a.bias[a.w_row[g] + c] : 0.f;
    }
    const int yoff = a.y_off[g];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int oy = y0 + wave * 2 + (b >> 1), ox = x0 + (b & 1) * 16 + row;
        if (oy < a.H && ox < a.W) {
            uint16_t *yp = a.y + (img + (size_t)oy * a.W + ox) * a.Cy + yoff;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = kq * 4 + j;
                float f = acc[b][j] + bs[j];
                if (a.relu) f = fmaxf(f, 0.f);
                if (c < cout) yp[c] = f2bf_finite(f);
            }
        }
    }
}

template <int KS>
constexpr int grouped_lds() { return (GC_TH + 2 * (KS / 2)) * (GC_TW + 2 * (KS / 2)) * 128; }

}  // namespace md

using namespace md;

// in : x[N,H,W,C] bf16, w[R, k*k*64] bf16, bias[R] f32 ; out: y[N,H,W,Cy] bf16.  extra: md_conv2d_grouped_attrs (required).
// Every check precedes the first device call.
extern "C" int md_conv2d_grouped(MD_AOT_ARGS) {
    Args g(MD_ARGS, 4, 4);
    const md_conv2d_grouped_attrs *at = g.attrs<md_conv2d_grouped_attrs>(extra);
    g.tensor(0, BF16, 4); g.tensor(1, BF16, 2); g.tensor(2, F32, 1); g.tensor(3, BF16, 4);
    if (int rc = g.rc()) return rc;
    if (at->reserved0 != 0) return MD_ERR_ARG;
    if (at->k != 1 && at->k != 3) return MD_ERR_ARG;
    if (at->relu != 0 && at->relu != 1) return MD_ERR_ARG;
    if (at->cin_g != 64) return MD_ERR_ARG;
    const int G = at->groups;
    if (G < 1 || G > MD_GROUPED_MAX_GROUPS) return MD_ERR_ARG;
    const int64_t N = g.d(0, 0), H = g.d(0, 1), W = g.d(0, 2), C = g.d(0, 3);
    const int64_t R = g.d(1, 0), Cy = g.d(3, 3);
    if (N < 0 || H < 0 || W < 0 || C % 8 || Cy % 8 || Cy <= 0) return MD_ERR_ARG;
    if (g.d(1, 1) != (int64_t)at->k * at->k * 64 || g.d(2, 0) != R) return MD_ERR_ARG;
    if (g.d(3, 0) != N || g.d(3, 1) != H || g.d(3, 2) != W) return MD_ERR_ARG;
    if (at->x_c_off < 0 || at->x_c_off % 8 || at->x_c_off + (int64_t)G * 64 > C) return MD_ERR_ARG;
    for (int g = 0; g < G; ++g) {
        const int co = at->cout[g], yo = at->y_off[g], wr = at->w_row[g];
        if (co < 1 || co > 16 || yo < 0 || yo + co > Cy || wr < 0 || wr + co > R) return MD_ERR_ARG;
        for (int h = 0; h < g; ++h)   // two groups writing one channel would race
            if (yo < at->y_off[h] + at->cout[h] && at->y_off[h] < yo + co) return MD_ERR_ARG;
    }
    if (mul({N, H, W}) == 0) return MD_OK;
    if (!g.have({0, 1, 2, 3})) return MD_ERR_ARG;
    {   // y must not overlap x (a workgroup's halo pixels are other workgroups' outputs)
        const char *xb = (const char *)params[0], *yb = (const char *)params[3];
        const long long xn = mul({N, H, W, C, 2}), yn = mul({N, H, W, Cy, 2});
        if (ranges_overlap(xb, xn, yb, yn)) return MD_ERR_ARG;
    }
    if (H > 32000 || W > 32000 || C > 65536 || Cy > 65536) return MD_ERR_SIZE;
    GroupedArgs a;
    a.x = (const uint16_t *)params[0]; a.w = (const uint16_t *)params[1]; a.bias = (const float *)params[2]; a.y = (uint16_t *)params[3];
    a.N = (int)N; a.H = (int)H; a.W = (int)W; a.C = (int)C; a.Cy = (int)Cy; a.G = G;
    a.x_c_off = at->x_c_off; a.relu = at->relu;
    a.tiles_x = (int)((W + GC_TW - 1) / GC_TW); a.tiles_y = (int)((H + GC_TH - 1) / GC_TH);
    const long long n_work = N * a.tiles_x * a.tiles_y * (long long)G;
    if (!fits_i32(n_work * 2)) return MD_ERR_SIZE;
    a.n_work = (int)n_work;
    a.work_per_xcd = (a.n_work + 7) / 8;
    for (int g = 0; g < MD_GROUPED_MAX_GROUPS; ++g) {
        a.cout[g] = g < G ? at->cout[g] : 0;
        a.y_off[g] = g < G ? at->y_off[g] : 0;
        a.w_row[g] = g < G ? at->w_row[g] : 0;
    }
    void (*k)(GroupedArgs) = at->k == 3 ? grouped_conv_kernel<3> : grouped_conv_kernel<1>;
    const int lds = at->k == 3 ? grouped_lds<3>() : grouped_lds<1>();
    if (ensure_dyn_lds((const void *)k, lds) != MD_OK) return MD_ERR_HIP;
    hipLaunchKernelGGL(k, dim3((unsigned)a.work_per_xcd * 8u), dim3(GC_THREADS), lds, (hipStream_t)stream, a);
    md_note_conv_kernel(MD_CONV_KERNEL_GROUPED);
    return launched();
}
