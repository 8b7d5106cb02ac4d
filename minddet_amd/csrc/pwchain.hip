// pwchain.hip -- md_pw_chain: conv3 (1x1, 128 -> 512) + residual + ReLU of one ResNet bottleneck block and conv1 (1x1, 512 -> 128) + ReLU of
// the next block in ONE launch (include/minddet_hip_chain.h).
//
// Why: at every identity-block boundary of ResNet stage 2 the 512-channel tensor y is written by conv3 and read twice by the next block,
// as its residual and by its conv1.  Both layers are HBM-bound and already run near copy speed, so only their bytes can go: per pixel
// conv3 moves 256 (t2) + 1024 (residual) + 1024 (y) bytes and conv1 1024 (y) + 256 (t1) = 3584; with conv1 computed from the y tile while
// it is on chip 2560 remain.
//
// Scheme: conv1x1_stream_kernel's (conv.hip), weight-stationary, with a second GEMM behind the epilogue.  One 8-wave workgroup per CU
// streams consecutive 32-pixel tiles past weights that never leave its registers:
//   * wave w keeps conv3 rows 64 w .. 64 w + 63 x K = 128 (64 registers) and conv1 rows 16 w .. 16 w + 15 x K = 512 (64 registers);
//   * t2 comes through a 4-slot LDS-DMA ring (8 KiB per slot) requested 3 tiles ahead, retired with a counted vmcnt + one raw s_barrier;
//   * the residual is DMAed one tile ahead straight into the wave's private 4-KiB epilogue image [32 px][64 couts]; the epilogue adds it in
//     place (each 8-byte cell is read and re-written by the same lane) and the image leaves as whole 128-B-line buffer stores;
//   * the eight wave images together ARE the y tile [32 px][512]: after one workgroup barrier every wave reads all eight as B fragments of
//     v_mfma_f32_16x16x32_bf16 for its 16 conv1 couts (the chip rounds this shape exactly as the 32x32x16 one the 128x128 kernel uses:
//     tools/pp_mf_ab.py; test_exact_regime_both_outputs_bit_for_bit of tests/test_pw_chain_gpu.py holds t1 to the float64 result bit for
//     bit on integer data, independently of md_conv2d).  Two image sets: the next tile's residual lands in the other set
//     while GEMM 2 reads this one;
//   * t1 is assembled as a [32 px][128] tile in LDS and leaves as whole 256-B rows one barrier later (under the next tile's GEMM 1).
// Every global access goes through a buffer descriptor re-based per tile with 64-bit scalar math: rows past M read zeros / drop their
// stores by the hardware range check, and no tensor-size limit applies.  A tile index outside the workgroup's range gets an EMPTY
// descriptor and its DMAs / stores are still issued, so every wave's vector-memory queue has the same shape in every iteration and the
// waits are compile-time counts.  No two workgroups touch a common byte, so their placement on the XCDs does not matter.
// Rounds exactly where the two md_conv2d launches round (conv + bias -> bf16, + residual -> bf16, ReLU; conv1 reads the bf16 y).
// Held to float64 by tests/test_pw_chain_gpu.py against conv_contract.reference_pw_chain: y and t1 bit for bit in the exact regime, each
// within one conv's derived bound in the Gaussian regime, at workgroup tile counts of 1 to 5 (below, at and above the look-ahead).
//
// LDS: ring 32 KiB | 2 x 8 images 64 KiB | t1 tile 8 KiB | b3 2 KiB = 106 KiB (b1: four registers per lane).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aot.h"
#include "device.h"
#include "../../include/minddet_hip_chain.h"

namespace md {

struct ChainArgs {
    const uint16_t *t2, *res, *w3, *w1;
    const float *b3, *b1;
    uint16_t *y, *t1;
    long long M;       // pixels
    int n_tiles;       // 32-pixel tiles
};

#define MD_CHAIN_WAIT_VMCNT(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory")

constexpr int PC_PT = 32;                          // pixels per tile
constexpr int PC_NR = 4, PC_D = PC_NR - 1;         // t2 ring slots, tiles of look-ahead
constexpr int PC_SLOT = PC_PT * 256;               // bytes per ring slot (32 px x 128 ch)
constexpr int PC_EW = PC_PT * 128;                 // bytes of a wave's image (32 px x 64 couts)
constexpr int PC_NE = PC_EW / 1024;                // 1-KiB pieces of an image = residual DMAs = y stores per wave and tile
constexpr int PC_SET = 8 * PC_EW;                  // one y tile
constexpr int PC_T1 = PC_PT * 256;                 // the t1 tile (32 px x 128 ch)
constexpr int PC_OFF_Y = PC_NR * PC_SLOT, PC_OFF_T1 = PC_OFF_Y + 2 * PC_SET, PC_OFF_BIAS = PC_OFF_T1 + PC_T1;
constexpr int PC_LDS = PC_OFF_BIAS + 512 * 4;
constexpr int PC_PER_ITER = 1 + 1 + 2 * PC_NE;     // vector-memory operations a wave issues per tile: t2 piece, t1 store, residual, y

__global__ __launch_bounds__(512, 1) void pw_chain_kernel(ChainArgs a) {
    typedef __attribute__((address_space(3))) void lds_void;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *ring = smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;      // 32x32x16 fragment row / k half
    const int p16 = lane & 15, q = lane >> 4;      // 16x16x32 fragment row / k quarter
    char *Y = smem + PC_OFF_Y + wave * PC_EW;      // this wave's image of set 0
    char *T1 = smem + PC_OFF_T1;
    float *bias_lds = reinterpret_cast<float *>(smem + PC_OFF_BIAS);

    // this workgroup's consecutive tiles: the first (n_tiles % grid) workgroups take one more
    const int G = gridDim.x, per = a.n_tiles / G, extra = a.n_tiles % G, g = blockIdx.x;
    const int t0 = g * per + (g < extra ? g : extra);
    const int nt = per + (g < extra ? 1 : 0);
    const int cout_w = wave * 64;                  // this wave's first conv3 output channel

    // ---- per-lane offsets, constant for the whole launch
    const int xrow = wave * 4 + (lane >> 4);
    const unsigned xoff = (unsigned)(xrow * 256 + (((lane & 15) ^ (xrow & 15)) << 4));   // t2 piece of this wave: 4 tile rows, source chunk swizzled
    unsigned eoff[PC_NE];                          // image piece i: row = 8 i + lane / 8, physical chunk lane % 8 holds logical chunk ^ swizzle
#pragma unroll
    for (int i = 0; i < PC_NE; ++i) {
        const int row = i * 8 + (lane >> 3), lc = (lane & 7) ^ ((row >> 1) & 7);
        eoff[i] = (unsigned)(row * 1024 + lc * 16);
    }
    int foff[8];                                   // GEMM 1 B fragment of k-step s: ring slot + foff[s]
#pragma unroll
    for (int s = 0; s < 8; ++s) foff[s] = lr * 256 + (((2 * s + lh) ^ (lr & 15)) << 4);
    const int eswz = (lr >> 1) & 7;
    int g2off[2];                                  // GEMM 2 B fragment of k-step ks, pixel block pb: set + (ks >> 1) * 4 KiB + pb * 2 KiB + g2off[ks & 1]
#pragma unroll
    for (int h = 0; h < 2; ++h) g2off[h] = p16 * 128 + (((h * 4 + q) ^ ((p16 >> 1) & 7)) << 4);
    // t1 tile [32 px][16 chunks of 8 ch], chunk index XOR (row & 15): written as 8-byte cells in accumulator layout, read out as 16-B chunks
    const int t1w = p16 * 256 + (((2 * wave + (q >> 1)) ^ p16) << 4) + (q & 1) * 8;    // pixel block pb: + pb * 4 KiB
    const int t1row = wave * 4 + (lane >> 4);
    const unsigned t1off = (unsigned)(t1row * 256 + (((lane & 15) ^ (t1row & 15)) << 4));

    // ---- per-tile descriptors (scalar)
    auto clip = [](long long rem) { return (int)(rem > 0x7fffffffLL ? 0x7fffffffLL : (rem < 0 ? 0 : rem)); };
    auto x_desc = [&](int t) {
        const bool live = t < nt;
        const long long m0 = live ? (long long)(t0 + t) * PC_PT : 0;
        return srd(a.t2 + m0 * 128, clip(live ? (a.M - m0) * 256 : 0));
    };
    auto r_desc = [&](int t) {
        const bool live = t < nt;
        const long long m0 = live ? (long long)(t0 + t) * PC_PT : 0;
        return srd(a.res + m0 * 512 + cout_w, clip(live ? (a.M - m0) * 1024 - cout_w * 2 : 0));
    };
    auto y_desc = [&](int t) {
        const long long m0 = (long long)(t0 + t) * PC_PT;
        return srd(a.y + m0 * 512 + cout_w, clip((a.M - m0) * 1024 - cout_w * 2));
    };
    auto t1_desc = [&](int t) {
        const bool live = t >= 0;
        const long long m0 = live ? (long long)(t0 + t) * PC_PT : 0;
        return srd(a.t1 + m0 * 128, clip(live ? (a.M - m0) * 256 : 0));
    };
    auto dma_x = [&](int t, int slot) {
        __amdgpu_buffer_rsrc_t rs = x_desc(t);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void *)(ring + slot * PC_SLOT + wave * 1024), 16, (int)xoff, 0, 0, 0);
    };
    auto dma_res = [&](int t, int set) {
        __amdgpu_buffer_rsrc_t rs = r_desc(t);
#pragma unroll
        for (int i = 0; i < PC_NE; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void *)(Y + set * PC_SET + i * 1024), 16, (int)eoff[i], 0, 0, 0);
    };

    // ---- prologue: the first D t2 tiles and the first residual tile are requested BEFORE the weights
#pragma unroll
    for (int t = 0; t < PC_D; ++t) dma_x(t, t);
    dma_res(0, 0);
    bias_lds[tid] = a.b3[tid];
    bf16x8 wr[2][8];        // conv3: A fragments of 32x32x16, rows cout_w + 32 b + lr, k = 16 s + 8 lh
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int s = 0; s < 8; ++s) wr[b][s] = *reinterpret_cast<const bf16x8 *>(a.w3 + (size_t)(cout_w + b * 32 + lr) * 128 + s * 16 + lh * 8);
    bf16x8 w1r[16];         // conv1: A fragments of 16x16x32, rows 16 wave + p16, k = 32 ks + 8 q
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) w1r[ks] = *reinterpret_cast<const bf16x8 *>(a.w1 + (size_t)(wave * 16 + p16) * 512 + ks * 32 + q * 8);
    const f32x4 b1v = *reinterpret_cast<const f32x4 *>(a.b1 + wave * 16 + q * 4);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int s_cur = 0, s_new = PC_D, set = 0;   // ring slot of tile t / of tile t + D; image set of tile t
    for (int t = 0; t < nt; ++t) {
        // t2 tile t was requested D iterations ago; behind its piece in this wave's queue: the rest of that iteration and D - 1 whole ones
        __builtin_amdgcn_sched_barrier(0);
        MD_CHAIN_WAIT_VMCNT(PC_D * PC_PER_ITER - 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();       // tile t is in the ring; every wave is past GEMM 2 of tile t - 1 and has written its t1 cells
        __builtin_amdgcn_sched_barrier(0);
        dma_x(t + PC_D, s_new);             // that slot was last read by GEMM 1 of tile t - 1
        {   // t1 of tile t - 1 leaves as whole 256-B rows (t = 0: empty descriptor, the store is dropped)
            __amdgpu_buffer_rsrc_t rt = t1_desc(t - 1);
            u32x4 v = *reinterpret_cast<const u32x4 *>(T1 + wave * 1024 + lane * 16);
            MD_BUFFER_STORE_B128(v, rt, t1off, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        dma_res(t + 1, set ^ 1);            // the other set was last read by GEMM 2 of tile t - 1
        __builtin_amdgcn_sched_barrier(0);

        // ---- GEMM 1: acc[64 couts of this wave][32 px] = W3 . t2
        const char *S = ring + s_cur * PC_SLOT;
        f32x16 acc[2];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;
        bf16x8 fb[2];
        fb[0] = *reinterpret_cast<const bf16x8 *>(S + foff[0]);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (s + 1 < 8) fb[(s + 1) & 1] = *reinterpret_cast<const bf16x8 *>(S + foff[s + 1]);
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wr[b][s], fb[s & 1], acc[b], 0, 0, 0);
        }
        s_cur = (s_cur + 1) & (PC_NR - 1);
        s_new = (s_new + 1) & (PC_NR - 1);

        // ---- epilogue 1 on the wave's private image.  bf16(acc + bias) first: it needs no residual and runs under the wait below
        char *E = Y + set * PC_SET;
        u32x2 pk[2][4];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            f32x4 bv[4];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) bv[gq] = *reinterpret_cast<const f32x4 *>(bias_lds + cout_w + b * 32 + 8 * gq + 4 * lh);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const f32x2 s01 = (f32x2){acc[b][4 * gq + 0], acc[b][4 * gq + 1]} + (f32x2){bv[gq].x, bv[gq].y};
                const f32x2 s23 = (f32x2){acc[b][4 * gq + 2], acc[b][4 * gq + 3]} + (f32x2){bv[gq].z, bv[gq].w};
                pk[b][gq].x = pk_bf16(s01.x, s01.y);
                pk[b][gq].y = pk_bf16(s23.x, s23.y);
            }
        }
        // the residual was requested one iteration ago; behind it in the queue: that iteration's y stores and this one's t2 piece, t1
        // store and residual pieces.  It is added in place, each 8-byte cell read and re-written by the same lane.  Builtin vector types
        // only on LDS while DMAs are pending (conv1x1_stream_kernel has the reason)
        __builtin_amdgcn_sched_barrier(0);
        MD_CHAIN_WAIT_VMCNT(PC_NE + 2 + PC_NE);
        __builtin_amdgcn_sched_barrier(0);
        u32x2 rv[2][4];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) rv[b][gq] = *reinterpret_cast<const u32x2 *>(E + lr * 128 + (((4 * b + gq) ^ eswz) << 4) + 8 * lh);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const f32x2 a01 = bf2f_pair(pk[b][gq].x) + bf2f_pair(rv[b][gq].x), a23 = bf2f_pair(pk[b][gq].y) + bf2f_pair(rv[b][gq].y);
                u32x2 o;
                o.x = pk_relu_bf16(pk_bf16(a01.x, a01.y));
                o.y = pk_relu_bf16(pk_bf16(a23.x, a23.y));
                *reinterpret_cast<u32x2 *>(E + lr * 128 + (((4 * b + gq) ^ eswz) << 4) + 8 * lh) = o;
            }
        __amdgpu_buffer_rsrc_t ry = y_desc(t);
        MD_WAVE_LDS_ORDER();   // the cells above were written by other lanes of this wave than the ones that read them out below
#pragma unroll
        for (int i = 0; i < PC_NE; ++i) {
            u32x4 v = *reinterpret_cast<const u32x4 *>(E + i * 1024 + lane * 16);
            MD_BUFFER_STORE_B128(v, ry, eoff[i], 0, 0);
        }

        // ---- GEMM 2: c2[16 couts of this wave][32 px] = W1 . y, y = the eight images of this set
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();       // the y tile is complete; every wave has read the t1 tile of tile t - 1 out
        __builtin_amdgcn_sched_barrier(0);
        const char *YT = smem + PC_OFF_Y + set * PC_SET;
        f32x4 c2[2];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) c2[pb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // B fragments two k-steps (four reads) ahead of the MFMAs that take them
        auto y_frag = [&](int ks, int pb) { return *reinterpret_cast<const bf16x8 *>(YT + (ks >> 1) * PC_EW + pb * 2048 + g2off[ks & 1]); };
        bf16x8 yb[2][2][2];
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) yb[0][k2][pb] = y_frag(k2, pb);
#pragma unroll
        for (int kg = 0; kg < 8; ++kg) {
            if (kg + 1 < 8) {
#pragma unroll
                for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
                    for (int pb = 0; pb < 2; ++pb) yb[(kg + 1) & 1][k2][pb] = y_frag(2 * (kg + 1) + k2, pb);
            }
            __builtin_amdgcn_sched_barrier(0);   // (hipcc otherwise sinks each read to its MFMA and exposes the LDS latency 16 times per tile)
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
                for (int pb = 0; pb < 2; ++pb)
                    c2[pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1r[2 * kg + k2], yb[kg & 1][k2][pb], c2[pb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            const f32x4 v = c2[pb] + b1v;
            u32x2 pk;
            pk.x = pk_relu_bf16(pk_bf16(v.x, v.y));
            pk.y = pk_relu_bf16(pk_bf16(v.z, v.w));
            *reinterpret_cast<u32x2 *>(T1 + pb * 4096 + t1w) = pk;
        }
        set ^= 1;
    }
    // ---- the last tile's t1
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    {
        __amdgpu_buffer_rsrc_t rt = t1_desc(nt - 1);
        u32x4 v = *reinterpret_cast<const u32x4 *>(T1 + wave * 1024 + lane * 16);
        MD_BUFFER_STORE_B128(v, rt, t1off, 0, 0);
    }
}

static bool ranges_overlap(const void *p, long long pn, const void *r, long long rn) {
    const char *pb = (const char *)p, *rb = (const char *)r;
    return pb < rb + rn && rb < pb + pn;
}

}  // namespace md

using namespace md;

extern "C" int md_pw_chain(MD_AOT_ARGS) {
    Args g(MD_ARGS, 8, 8);
    g.tensor(0, BF16, 4); g.tensor(1, BF16, 4); g.tensor(2, BF16, 2); g.tensor(3, F32, 1); g.tensor(4, BF16, 2); g.tensor(5, F32, 1);
    g.tensor(6, BF16, 4); g.tensor(7, BF16, 4);
    const int64_t N = g.d(0, 0), H = g.d(0, 1), W = g.d(0, 2);
    g.require(g.d(0, 3) == 128 && g.d(1, 3) == 512 && g.d(6, 3) == 512 && g.d(7, 3) == 128);
    g.require(g.d(2, 0) == 512 && g.d(2, 1) == 128 && g.d(3, 0) == 512 && g.d(4, 0) == 128 && g.d(4, 1) == 512 && g.d(5, 0) == 128);
    for (int i : {1, 6, 7}) g.require(g.d(i, 0) == N && g.d(i, 1) == H && g.d(i, 2) == W);
    g.require(N >= 0 && H >= 0 && W >= 0);
    if (int rc = g.rc()) return rc;
    if (mul({N, H, W}) == 0) return MD_OK;
    if (!g.have({0, 1, 2, 3, 4, 5, 6, 7})) return MD_ERR_ARG;
    if (!fits_i32(N) || !fits_i32(H) || !fits_i32(W) || !fits_i32(mul({N, H})) || !fits_i32(mul({N, H, W}))) return MD_ERR_SIZE;
    const long long M = mul({N, H, W});
    // the outputs overlap neither an input nor each other
    const long long nb[8] = {M * 256, M * 1024, 0, 0, 0, 0, M * 1024, M * 256};
    for (int o : {6, 7})
        for (int i : {0, 1})
            if (ranges_overlap(params[o], nb[o], params[i], nb[i])) return MD_ERR_ARG;
    if (ranges_overlap(params[6], nb[6], params[7], nb[7])) return MD_ERR_ARG;
    ChainArgs a;
    a.t2 = (const uint16_t *)params[0]; a.res = (const uint16_t *)params[1]; a.w3 = (const uint16_t *)params[2]; a.b3 = (const float *)params[3];
    a.w1 = (const uint16_t *)params[4]; a.b1 = (const float *)params[5]; a.y = (uint16_t *)params[6]; a.t1 = (uint16_t *)params[7];
    a.M = M;
    a.n_tiles = (int)((M + PC_PT - 1) / PC_PT);
    if (ensure_dyn_lds((const void *)pw_chain_kernel, PC_LDS) != MD_OK) return MD_ERR_HIP;
    // one round of workgroups, one per CU (256): the weights are loaded once per workgroup
    const unsigned grid = a.n_tiles < 256 ? (unsigned)a.n_tiles : 256u;
    hipLaunchKernelGGL(pw_chain_kernel, dim3(grid), dim3(512), PC_LDS, (hipStream_t)stream, a);
    return launched();
}
