// bottleneck.hip -- a whole ResNet bottleneck block (stride 1, 64 mid channels) in ONE launch.
//
// What it replaces: Bottleneck.construct of minddet/models/centernet/src/resnet.py:139-178 --
//   conv1 1x1 (Cin -> 64) + bn1 + relu -> conv2 3x3 (64 -> 64) + bn2 + relu -> conv3 1x1 (64 -> 256) + bn3, + residual, relu --
// which md_conv2d runs as three launches that move 2048 B of activations per pixel through HBM (x read by conv1 AND again as the
// residual, the two 64-channel intermediates written and re-read).  Measured r01/r02 (profiles/): those launches already run at
// 5.2-5.8 TB/s of algorithmic traffic, i.e. at what the HBM gives -- only removing bytes makes the R50 / R101 stage-1 blocks
// faster.  Here a workgroup owns an 8 x 16 block of output pixels of one image and keeps everything between x and y on the CU:
//
//   phase A  T1[10x18 halo px][64] = relu(W1 . x + b1), zero outside the image (the 3x3 conv's zero padding applies to T1);
//            x streams through LDS in 64-channel chunks (LDS-DMA, two buffers, counted vmcnt, raw s_barrier), T1 stays in LDS
//   phase B  T2[8x16 px][64] = relu(sum_taps W2[tap] . T1[shifted rows] + b2): the halo-reuse scheme of conv3x3_halo_kernel with
//            the halo read from T1 instead of from HBM; only the 8 KiB weight slice of each tap is streamed (from L2)
//   phase C  y[px][256] = relu(W3 . T2 + b3 + residual): wave (wc, wq) owns output quarters 2 wc, 2 wc + 1 (64 channels each) of its 32
//            pixels and moves them through a wave-PRIVATE 16-pixel x 64-channel slab -- no workgroup barrier in the whole phase (r03;
//            the r02 form synchronised all 8 waves twice per quarter around a shared image: 9.4 k of a tile's 31.9 k cycles) -- out as
//            whole 128-B-line buffer stores; the residual is the block input (copied out of the x chunks while they sit in LDS), a
//            separate tensor, or the fused downsample conv's values held in registers.
//
// HBM traffic per pixel: 512 B in (+ the halo columns that miss L2) + 512 B out instead of 2048 B.  Per 128-pixel tile: 604
// v_mfma_f32_32x32x16_bf16 (19.8 MFLOP) against 128 KiB of HBM traffic = 155 flop/B: the block is HBM-bound as long as the
// matrix pipe runs above 33 % busy, which two resident workgroups per CU (80 KiB of LDS each) provide.
//
// LDS map (80 KiB): A [0,32K) phase A: W1 chunk a (8K) + x chunk a (24K) | B: W2 taps 0-3 / 5-8 | C: W3 (32K)
//                   B [32K,56K) phase A: x chunk b | B: T1 | C: transpose image (18K)
//                   C [56K,64K) phase A: W1 chunk b | B: W2 tap 4 | C: b3 (1K)
//                   D [64K,80K) phase A / B: b1, b2 (512 B) | C: T2 (16K)
// Tiles are [row][64 k] bf16 (128-B rows), the 16-B chunk index XOR-swizzled by (row >> 1) & 7 on the DMA's SOURCE chunk and on
// the fragment reads (conflict-free ds_read_b128), as in conv.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "aot.h"
#include "device.h"

namespace md {

struct BottleneckArgs {
    const uint16_t *x;    // [N,H,W,Cin]
    const uint16_t *w1;   // [64][Cin]
    const uint16_t *w2;   // [64][576]  K = tap * 64 + ci
    const uint16_t *w3;   // [256][64]
    const uint16_t *res;  // [N,H,W,256] (the block input when Cin == 256)
    const float *b1, *b3;   // b1: 128 floats = b1 | b2
    const uint16_t *wd;   // MODE 2: the downsample conv's [256][64] weights
    const float *bd;      // MODE 2: its 256 biases
    uint16_t *y;          // [N,H,W,256]
    int N, H, W, Cin, nch;            // nch = Cin / 64
    int tiles_x, tiles_y, n_tiles, pt_per_xcd;
    unsigned x_bytes, w1_bytes;
    unsigned long long *dbg;   // MD_DIAG builds only
};

constexpr int BN_TH = 8, BN_TW = 16, BN_HW = BN_TW + 2, BN_HALO = (BN_TH + 2) * BN_HW;  // 180 halo pixels
constexpr int BN_ROWB = 128;
constexpr int BN_A = 0, BN_B = 32768, BN_C = 57344, BN_D = 65536, BN_LDS = 81920;
constexpr int BN_ES = 144;  // transpose image row stride (64 channels * 2 B + 16)

// MD_DIAG build (tools/bottleneck_stamps.py): cycle stamps of one mid-grid workgroup, written to a buffer of their own
#ifdef MD_DIAG
#define BN_STAMP(I) do { if (a.dbg) { __builtin_amdgcn_sched_barrier(0); stp[I] = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#else
#define BN_STAMP(I) do { } while (0)
#endif
#define BN_BAR_RAW()                                              \
    do {                                                          \
        __builtin_amdgcn_sched_barrier(0);                        \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        \
        __builtin_amdgcn_s_barrier();                             \
        __builtin_amdgcn_sched_barrier(0);                        \
    } while (0)

// MODE 0: the residual is the block input itself (Cin == 256): output quarter q's residual channels are exactly x chunk q, so each
//         thread copies its 16-B pieces out of the chunk while it sits in LDS (no second trip to L2 / HBM, no latency in phase C).
// MODE 1: the residual is a separate [N,H,W,256] tensor, requested behind the last DMA of the tile.
// MODE 2: the residual is the block's 1x1 downsample conv of x (Cin == 64: the first block of a stage, resnet.py:214-224 /
//         _make_layer): Wd (32 KiB) is staged beside the one x chunk and phase A also computes bf16(Wd . x + bd) for the tile's 128
//         centre pixels -- each wave exactly the (cout fragment, pixel fragment) tiles it owns again in phase C, so the values stay
//         in 32 registers in accumulator layout; neither the downsample launch nor its 512 B / pixel output exist any more.
// All three round where the layer-by-layer path rounds (conv3 -> bf16, residual -> bf16, sum -> bf16): bit-identical to it.
// 8 waves per workgroup, two workgroups per CU = 4 waves per SIMD: r02 stamps (tools/bottleneck_stamps.py) of the 4-wave form showed
// every phase latency-bound at 2 waves per SIMD (27 % MFMA-busy, HBM traffic already at the algorithmic minimum).
constexpr bool M2_SLAB = false;   // MODE 2 on the slab form of phase C: 2 spilled registers at the 128-register budget (scratch costs ~7 %): off
template <int MODE>
__global__ __launch_bounds__(512, 4) void bottleneck64_kernel(BottleneckArgs a) {
    typedef __attribute__((address_space(3))) void lds_void;
    constexpr unsigned OOR = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    // lane -> pixel of the wave's 32-pixel fragment (= two 16-pixel tile rows, 18 halo rows apart) wherever the pixel operand is read at
    // tap-shifted halo rows (phase B; MODE 2's downsample conv): ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}
    // {4-11, 16-19, 28-31} (+32); with pixel = lane a group straddles the two tile rows and two of its 16 halo rows coincide mod 16 = a 2-way
    // bank conflict on every such read (r03, tools/pmc_lds_survey.sh: conflict cycles = 0.9 x the LDS-busy cycles).  hp gives each group one
    // whole tile row.  T2 is stored at row = LANE, so phase C reads consecutive rows and its accumulator column lr is pixel hp as well.
    // (recomputed at each use behind an opaque copy of lr: held in a register across the phases it cost MODE 2 two spilled registers)
    auto hp_now = [&]() {
        int l = lr;
        asm volatile("" : "+v"(l));
        return (int)(((0x73261540u >> ((l >> 2) * 4)) & 7u) << 2) | (l & 3);   // 4-lane blocks 0..7 -> 0, 4, 5, 1, 6, 2, 3, 7 (branch-free)
    };
    const int wc = wave & 1, wq = wave >> 1;   // cout fragment (32 rows) / pixel-row fragment group of this wave
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int pt = xcd * a.pt_per_xcd + slot;
    if (pt >= a.n_tiles) return;
    const int tx = pt % a.tiles_x, ty = (pt / a.tiles_x) % a.tiles_y, n = pt / (a.tiles_x * a.tiles_y);
    const int y0 = ty * BN_TH, x0 = tx * BN_TW;
#ifdef MD_DIAG
    unsigned long long stp[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    BN_STAMP(0);

    __amdgpu_buffer_rsrc_t rs_x = srd(a.x, a.x_bytes);
    __amdgpu_buffer_rsrc_t rs_w1 = srd(a.w1, a.w1_bytes);
    __amdgpu_buffer_rsrc_t rs_w2 = srd(a.w2, 64 * 576 * 2);
    __amdgpu_buffer_rsrc_t rs_w3 = srd(a.w3, 256 * 64 * 2);
    __amdgpu_buffer_rsrc_t rs_wd = srd(MODE == 2 ? a.wd : a.w3, 256 * 64 * 2);

    // ---- staging maps.  One wave instruction = 8 rows x 128 B; lane -> (row = 8 * piece + lane / 8, physical chunk = lane & 7).
    // 64-row weight tiles = 8 pieces: wave w stages piece w.  x halo = 24 pieces: wave w stages pieces w, w + 8, w + 16.
    const int srow = lane >> 3;
    const int wrow = wave * 8 + srow;
    const int wchunk = (lane & 7) ^ ((wrow >> 1) & 7);
    unsigned h_off[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int r = (wave + 8 * j) * 8 + srow;
        const int hy = r / BN_HW, hx = r - hy * BN_HW;
        const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        const int lchunk = (lane & 7) ^ ((r >> 1) & 7);
        const bool ok = r < BN_HALO && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        h_off[j] = ok ? (unsigned)((((n * a.H + iy) * a.W + ix) * a.Cin + lchunk * 8) * 2) : OOR;
    }
    // biases: requested now (after the address arithmetic above: hipcc otherwise parks a load's destination in the don't-care half
    // of a 64-bit multiply-add operand and waits for the load in front of the first DMA), parked in LDS later (b1 | b2 in region D,
    // b3 in region C)
    __builtin_amdgcn_sched_barrier(0);
    const float b3_early = a.b3[tid & 255];
    const float b12_early = a.b1[tid & 127];   // b1 | b2 are 64 + 64 consecutive floats (the host packs them so)
    float bd_early = 0.f;
    if constexpr (MODE == 2) bd_early = a.bd[tid & 255];
    __builtin_amdgcn_sched_barrier(0);
    auto dma_chunk_a = [&](int kt, int buf) {   // phase A: chunk kt of W1 (64 x 64) and of the x halo (192 x 64): 4 instructions per wave
        char *Wd = smem + (buf ? BN_C : BN_A), *Xd = smem + (buf ? BN_B : BN_A + 8192);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w1, (lds_void *)(Wd + wave * 1024), 16, (wrow * a.Cin + wchunk * 8) * 2, kt * 128, 0, 0);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_void *)(Xd + (wave + 8 * j) * 1024), 16, (int)h_off[j], kt * 128, 0, 0);
    };
    auto dma_tap = [&](int t, char *dst) {      // phase B: W2[:, tap t] (64 x 64): 1 instruction per wave
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w2, (lds_void *)(dst + wave * 1024), 16, (wrow * 576 + wchunk * 8) * 2, t * 128, 0, 0);
    };

    // ---- phase A: T1 = relu(W1 . x + b1) on the 192 halo rows = 2 cout x 6 row fragments of 32 x 32: wave (wc, wq) owns row
    // fragments wq and, for wq < 2, wq + 4
    const bool two = wq < 2;
    f32x16 acc1[2];
    // phase C ownership: wave (wc, wq) = output quarters 2 wc + {0, 1} x pixels 32 wq .. + 31.  This lane's four 16-B pieces of a quarter
    // (the read-out of the wave's 16-pixel slab, twice): piece i = h * 2 + it -> pixel 32 wq + 16 h + 8 it + lane / 8, 16-B chunk lane & 7
    u32x4 rres[MODE == 2 ? 1 : 2][MODE == 2 ? 1 : 4];
    int res_lds[4] = {0, 0, 0, 0};   // IDENT: where that piece of the residual sits in an x chunk (halo row of the centre pixel, swizzled chunk)
    if constexpr (MODE == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = 32 * wq + 8 * i + (lane >> 3), cc = lane & 7;
            const int r = ((p >> 4) + 1) * BN_HW + (p & 15) + 1;
            res_lds[i] = swz128(r, cc);
        }
    }
    dma_chunk_a(0, 0);
    if (a.nch > 1) dma_chunk_a(1, 1);
    if constexpr (MODE == 2) {   // Wd (256 x 64) -> regions B + C (buffer b is idle: one chunk only): 32 pieces, 4 per wave
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = (wave + 8 * j) * 8 + srow;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_wd, (lds_void *)(smem + BN_B + (wave + 8 * j) * 1024), 16,
                                                     (row * 64 + ((lane & 7) ^ ((row >> 1) & 7)) * 8) * 2, 0, 0, 0);
        }
    }
    float *bias12 = reinterpret_cast<float *>(smem + BN_D);
    if (tid < 128) bias12[tid] = b12_early;   // the load is older than every DMA: waiting for it drains nothing
    if (MODE == 2 && tid < 256) bias12[128 + tid] = bd_early;
    unsigned resd[4][8];   // MODE 2: bf16(Wd . x + bd) of this wave's four (cout fragment, pixel fragment) tiles, accumulator layout
    for (int kt = 0; kt < a.nch; ++kt) {
        // this wave's share of chunk kt has landed; the 4 younger DMAs (chunk kt + 1, or the W2 taps requested below) stay in flight
        if (kt + 1 < a.nch || a.nch >= 3) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        BN_BAR_RAW();
        if (kt == 0) BN_STAMP(1);
        const char *Wt = smem + ((kt & 1) ? BN_C : BN_A), *Xt = smem + ((kt & 1) ? BN_B : BN_A + 8192);
        if constexpr (MODE == 2) {   // the downsample conv on the centre pixels (kt == 0 is the only chunk)
            const int pc_ = 32 * wq + hp_now();
            const int rc = ((pc_ >> 4) + 1) * BN_HW + (pc_ & 15) + 1;   // halo row of this lane's centre pixel
            bf16x8 fx[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) fx[kk] = *reinterpret_cast<const bf16x8 *>(Xt + swz128(rc, 2 * kk + lh));
#pragma unroll
            // (the row expressions are written out in place: a hoisted `row0 = 64 q + 32 wc` cost this instantiation 9 spilled registers, and
            // with scratch in use the kernel ran 7 % slower -- r03, found by bisecting against the round-2 source)
            for (int q = 0; q < 4; ++q) {   // the (quarter, cout fragment) tiles this wave owns again in phase C: M2_SLAB: cout rows
                                            // 64 (2 wc + q / 2) + 32 (q & 1) .., else 64 q + 32 wc ..
                f32x16 accd;
#pragma unroll
                for (int e = 0; e < 16; ++e) accd[e] = 0.f;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const bf16x8 fa = *reinterpret_cast<const bf16x8 *>(smem + BN_B + swz128((M2_SLAB ? 64 * (2 * wc + (q >> 1)) + 32 * (q & 1) : 64 * q + 32 * wc) + lr, 2 * kk + lh));
                    accd = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fx[kk], accd, 0, 0, 0);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias12 + 128 + (M2_SLAB ? 64 * (2 * wc + (q >> 1)) + 32 * (q & 1) : 64 * q + 32 * wc) + 8 * g + 4 * lh);
                    resd[q][2 * g + 0] = pk_bf16(accd[4 * g + 0] + bv.x, accd[4 * g + 1] + bv.y);
                    resd[q][2 * g + 1] = pk_bf16(accd[4 * g + 2] + bv.z, accd[4 * g + 3] + bv.w);
                }
                __builtin_amdgcn_sched_barrier(0);   // keeps hipcc from hoisting all four quarters' fragment reads (register budget)
            }
        }
        if (kt == 0) {   // (zeroed here, behind the MODE 2 block: its accumulators and these are then never live together)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc1[j][e] = 0.f;
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const bf16x8 fa = *reinterpret_cast<const bf16x8 *>(Wt + swz128(32 * wc + lr, 2 * kk + lh));
            const bf16x8 fb0 = *reinterpret_cast<const bf16x8 *>(Xt + swz128(32 * wq + lr, 2 * kk + lh));
            acc1[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb0, acc1[0], 0, 0, 0);
            if (two) {
                const bf16x8 fb1 = *reinterpret_cast<const bf16x8 *>(Xt + swz128(32 * (wq + 4) + lr, 2 * kk + lh));
                acc1[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb1, acc1[1], 0, 0, 0);
            }
        }
        if constexpr (MODE == 0) {   // x chunk kt = the residual channels of output quarter kt: copied by the waves that own that quarter
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q == kt && (q >> 1) == wc) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) rres[q & 1][i] = *reinterpret_cast<const u32x4 *>(Xt + res_lds[i]);
                }
        }
        BN_BAR_RAW();   // every wave has finished reading this buffer
        if (kt + 2 < a.nch) dma_chunk_a(kt + 2, kt & 1);
        else if (a.nch >= 3 && kt == a.nch - 2) {
            // buffer a (region A) has seen its last chunk: W2 taps 0-3 are requested now and land behind the last chunk's MFMAs
            // (nch is even here: chunk nch - 2 used buffer a; the host side admits nch = 1 or 4)
#pragma unroll
            for (int t = 0; t < 4; ++t) dma_tap(t, smem + BN_A + t * 8192);
        }
    }
    BN_STAMP(2);
    // W2 taps 0-3 -> region A (if not requested above), tap 4 -> region C (free: the loop's last barrier has passed)
    if (a.nch < 3) {
#pragma unroll
        for (int t = 0; t < 4; ++t) dma_tap(t, smem + BN_A + t * 8192);
    }
    dma_tap(4, smem + BN_C);
    {   // T1 -> region B: bias, ReLU, zero outside the image, bf16; lane = halo row, 4 consecutive channels per register group
        char *T1 = smem + BN_B;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j == 1 && !two) break;
            const int r = 32 * (wq + 4 * j) + lr;
            const int hy = r / BN_HW, hx = r - hy * BN_HW;
            const bool ok = r < BN_HALO && (unsigned)(y0 - 1 + hy) < (unsigned)a.H && (unsigned)(x0 - 1 + hx) < (unsigned)a.W;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c_local = 32 * wc + 8 * g + 4 * lh;
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias12 + c_local);
                u32x2 pk;
                pk.x = pk_relu_bf16(pk_bf16(acc1[j][4 * g + 0] + bv.x, acc1[j][4 * g + 1] + bv.y));
                pk.y = pk_relu_bf16(pk_bf16(acc1[j][4 * g + 2] + bv.z, acc1[j][4 * g + 3] + bv.w));
                if (!ok) pk.x = pk.y = 0u;
                *reinterpret_cast<u32x2 *>(T1 + r * BN_ROWB + (((4 * wc + g) ^ ((r >> 1) & 7)) << 4) + 8 * lh) = pk;
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    BN_STAMP(3);

    // ---- phase B: T2 = relu(conv3x3(T1) + b2) = 2 cout x 4 pixel fragments: wave (wc, wq) owns couts 32 wc.., pixels 32 wq..
    f32x16 acc2;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc2[e] = 0.f;
    const int pB = 32 * wq + hp_now();
    const int r0 = (pB >> 4) * BN_HW + (pB & 15);   // halo row of this lane's pixel for tap (0, 0)
    // a tap's eight fragments are requested together, then its four MFMAs run: one LDS round trip per tap (the other three waves of
    // the SIMD fill it); a second register set for cross-tap prefetch does not fit the 128-register budget of 4 waves per SIMD
    auto tap_mfma = [&](int t, const char *Wt) {
        const char *T1 = smem + BN_B;
        const int r = r0 + (t / 3) * BN_HW + (t % 3);
        const int sw = (r >> 1) & 7;
        bf16x8 tfa[4], tfb[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            tfb[kk] = *reinterpret_cast<const bf16x8 *>(T1 + r * BN_ROWB + (((2 * kk + lh) ^ sw) << 4));
            tfa[kk] = *reinterpret_cast<const bf16x8 *>(Wt + swz128(32 * wc + lr, 2 * kk + lh));
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tfa[kk], tfb[kk], acc2, 0, 0, 0);
    };
#pragma unroll
    for (int t = 0; t < 4; ++t) tap_mfma(t, smem + BN_A + t * 8192);
    tap_mfma(4, smem + BN_C);
    __syncthreads();   // taps 0-4 consumed
    BN_STAMP(4);
#pragma unroll
    for (int t = 5; t < 9; ++t) dma_tap(t, smem + BN_A + (t - 5) * 8192);
    if (tid < 256) reinterpret_cast<float *>(smem + BN_C)[tid] = b3_early;   // b3 -> region C (tap 4 is consumed)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    BN_STAMP(5);
#pragma unroll
    for (int t = 5; t < 9; ++t) tap_mfma(t, smem + BN_A + (t - 5) * 8192);
    f32x4 bv2[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bv2[g] = *reinterpret_cast<const f32x4 *>(bias12 + 64 + 32 * wc + 8 * g + 4 * lh);
    __syncthreads();   // every wave is done with T1, the tap buffers and b2
    BN_STAMP(6);
    // W3 (256 x 64) -> region A: 32 pieces, wave w stages pieces w + 8j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (wave + 8 * j) * 8 + srow;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w3, (lds_void *)(smem + BN_A + (wave + 8 * j) * 1024), 16,
                                                 (row * 64 + ((lane & 7) ^ ((row >> 1) & 7)) * 8) * 2, 0, 0, 0);
    }
    {   // T2 -> region D
        char *T2 = smem + BN_D;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            u32x2 pk;
            pk.x = pk_relu_bf16(pk_bf16(acc2[4 * g + 0] + bv2[g].x, acc2[4 * g + 1] + bv2[g].y));
            pk.y = pk_relu_bf16(pk_bf16(acc2[4 * g + 2] + bv2[g].z, acc2[4 * g + 3] + bv2[g].w));
            *reinterpret_cast<u32x2 *>(T2 + (32 * wq + lr) * BN_ROWB + (((4 * wc + g) ^ ((lr >> 1) & 7)) << 4) + 8 * lh) = pk;   // row = lane
        }
    }
    if constexpr (MODE == 2 && !M2_SLAB) {
    // ---- MODE 2 keeps the round-2 phase C (four 64-channel quarters through a shared 18-KiB transpose image, two raw barriers per quarter):
    // with the downsample conv's 32 value registers live, the slab form below needs more than the 128-register budget of four waves per SIMD
    // and measured 5.6 % slower on this block (r03, same box, tools/bottleneck_ab.py); the identity / residual-tensor blocks gain 2.1 % on it.
        // this thread's two 16-B pieces of a quarter's image in global memory
        long long g_off[2];
    #pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int e = tid + 512 * it, p = e >> 3, cc = e & 7;
            const int yy = y0 + (p >> 4), xx = x0 + (p & 15);
            g_off[it] = (yy < a.H && xx < a.W) ? ((long long)(n * a.H + yy) * a.W + xx) * 256 + cc * 8 : -1;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        BN_STAMP(7);

        // ---- phase C: y = relu(W3 . T2 + b3 + residual), 64 output channels at a time = 2 cout x 4 pixel fragments per quarter
        const float *bias3 = reinterpret_cast<const float *>(smem + BN_C);
        char *E = smem + BN_B;
        const int pE = 32 * wq + hp_now();   // the pixel of accumulator column lr
        // the pixel operand (T2 fragments) is the same for all four quarters: read once; the weight fragments of quarter q + 1 are
        // requested before quarter q's epilogue (W3 is read-only in this phase: no hazard with the image barriers)
        bf16x8 fbc[4], fac[2][4];
    #pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            fbc[kk] = *reinterpret_cast<const bf16x8 *>(smem + BN_D + swz128(32 * wq + lr, 2 * kk + lh));
            fac[0][kk] = *reinterpret_cast<const bf16x8 *>(smem + BN_A + swz128(32 * wc + lr, 2 * kk + lh));
        }
    #pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x16 acc3;
    #pragma unroll
            for (int e = 0; e < 16; ++e) acc3[e] = 0.f;
    #pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (q + 1 < 4) fac[(q + 1) & 1][kk] = *reinterpret_cast<const bf16x8 *>(smem + BN_A + swz128(64 * (q + 1) + 32 * wc + lr, 2 * kk + lh));
                acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fac[q & 1][kk], fbc[kk], acc3, 0, 0, 0);
            }
            if (q == 1) BN_STAMP(13);
    #pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c_local = 32 * wc + 8 * g + 4 * lh;
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias3 + 64 * q + c_local);
                u32x2 pk;
                pk.x = pk_bf16(acc3[4 * g + 0] + bv.x, acc3[4 * g + 1] + bv.y);
                pk.y = pk_bf16(acc3[4 * g + 2] + bv.z, acc3[4 * g + 3] + bv.w);
                if constexpr (MODE == 2) {   // + bf16(Wd . x + bd), ReLU: the final value goes into the image
                    const unsigned r0_ = resd[q][2 * g], r1_ = resd[q][2 * g + 1];
                    const f32x2 s0 = bf2f_pair(pk.x) + bf2f_pair(r0_), s1 = bf2f_pair(pk.y) + bf2f_pair(r1_);
                    pk.x = pk_relu_bf16(pk_bf16(s0.x, s0.y));
                    pk.y = pk_relu_bf16(pk_bf16(s1.x, s1.y));
                }
                *reinterpret_cast<u32x2 *>(E + pE * BN_ES + c_local * 2) = pk;
            }
            BN_BAR_RAW();   // raw barriers in this loop: __syncthreads() would wait for the previous quarter's stores to COMPLETE (vmcnt 0)
            if (q == 1) BN_STAMP(14);
    #pragma unroll
            for (int it = 0; it < 2; ++it) {
                if (g_off[it] < 0) continue;
                const int e = tid + 512 * it;
                u32x4 v = *reinterpret_cast<const u32x4 *>(E + (e >> 3) * BN_ES + (e & 7) * 16);
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(a.y + g_off[it] + 64 * q));
            }
            if (q == 1) BN_STAMP(15);
            BN_BAR_RAW();      // the image is rewritten by the next quarter
            BN_STAMP(8 + q);
        }
    } else {
        // this lane's four 16-B pieces of a quarter in global memory, as byte offsets behind the tile's first pixel (buffer descriptors based
        // there: 32-bit lane offsets, pixels outside the image dropped / read as zero by the hardware range check)
        constexpr unsigned OOR_Y = 0x80000000u;
        unsigned y_off[4];
    #pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = 32 * wq + 8 * i + (lane >> 3), cc = lane & 7;
            const int yy = y0 + (p >> 4), xx = x0 + (p & 15);
            y_off[i] = (yy < a.H && xx < a.W) ? (unsigned)((((p >> 4) * a.W + (p & 15)) * 256 + cc * 8) * 2) : OOR_Y;
        }
        const long long pix00 = ((long long)n * a.H + y0) * a.W + x0;
        const long long y_rem = ((long long)a.N * a.H * a.W - pix00) * 512;
        __amdgpu_buffer_rsrc_t rs_y = srd(a.y + pix00 * 256, (int)(y_rem > 0x7fffffffLL ? 0x7fffffffLL : y_rem));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        BN_STAMP(7);

        // ---- phase C: y = relu(W3 . T2 + b3 + residual); this wave: output quarters 2 wc, 2 wc + 1 of its 32 pixels, no workgroup barrier
        const float *bias3 = reinterpret_cast<const float *>(smem + BN_C);
        char *slab = smem + BN_B + wave * 2560;   // 16 pixels x 64 channels, 144-B rows (region B: T1 is consumed)
        if constexpr (MODE == 1) {   // a separate residual tensor: all 8 pieces requested now, behind every DMA of the tile
            __amdgpu_buffer_rsrc_t rs_r = srd(a.res + pix00 * 256, (int)(y_rem > 0x7fffffffLL ? 0x7fffffffLL : y_rem));
    #pragma unroll
            for (int q2 = 0; q2 < 2; ++q2)
    #pragma unroll
                for (int i = 0; i < 4; ++i)
                    rres[q2][i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_r, (int)y_off[i], (2 * wc + q2) * 128, 2));
        }
        // the pixel operand (T2 fragments) is the same for both quarters: read once
        bf16x8 fbc[4];
    #pragma unroll
        for (int kk = 0; kk < 4; ++kk) fbc[kk] = *reinterpret_cast<const bf16x8 *>(smem + BN_D + swz128(32 * wq + lr, 2 * kk + lh));
    #pragma unroll
        for (int q2 = 0; q2 < 2; ++q2) {
            const int q = 2 * wc + q2;   // output channels 64 q .. 64 q + 63
            // bias (+ the fused downsample conv's value, ReLU) -> bf16, in accumulator layout: lane = pixel hp, 4 consecutive channels per group.
            // One 32-channel fragment at a time (its accumulator dies into 8 packed registers before the next starts: register budget 128)
            unsigned pkv[2][8];
    #pragma unroll
            for (int f = 0; f < 2; ++f) {
                f32x16 acc3;
    #pragma unroll
                for (int e = 0; e < 16; ++e) acc3[e] = 0.f;
    #pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const bf16x8 fa = *reinterpret_cast<const bf16x8 *>(smem + BN_A + swz128(64 * q + 32 * f + lr, 2 * kk + lh));
                    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fbc[kk], acc3, 0, 0, 0);
                }
    #pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias3 + 64 * q + 32 * f + 8 * g + 4 * lh);
                    unsigned p0 = pk_bf16(acc3[4 * g + 0] + bv.x, acc3[4 * g + 1] + bv.y);
                    unsigned p1 = pk_bf16(acc3[4 * g + 2] + bv.z, acc3[4 * g + 3] + bv.w);
                    if constexpr (MODE == 2) {
                        const unsigned r0_ = resd[q2 * 2 + f][2 * g], r1_ = resd[q2 * 2 + f][2 * g + 1];
                        const f32x2 s0 = bf2f_pair(p0) + bf2f_pair(r0_), s1 = bf2f_pair(p1) + bf2f_pair(r1_);
                        p0 = pk_relu_bf16(pk_bf16(s0.x, s0.y));
                        p1 = pk_relu_bf16(pk_bf16(s1.x, s1.y));
                    }
                    pkv[f][2 * g] = p0; pkv[f][2 * g + 1] = p1;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (q2 == 0) BN_STAMP(13);
            const int hp = hp_now();
    #pragma unroll
            for (int h = 0; h < 2; ++h) {   // pixels 16 h .. 16 h + 15 of the wave's 32: the lanes with hp >> 4 == h hold them
                if ((hp >> 4) == h) {
    #pragma unroll
                    for (int f = 0; f < 2; ++f)
    #pragma unroll
                        for (int g = 0; g < 4; ++g)
                            *reinterpret_cast<u32x2 *>(slab + (hp & 15) * BN_ES + f * 64 + 16 * g + 8 * lh) = (u32x2){pkv[f][2 * g], pkv[f][2 * g + 1]};
                }
                // The slab is read back by OTHER lanes of the wave, in another vector type: without a compiler-level ordering point hipcc
                // duplicated the read-out into the lanes that skip the write block and ran it FIRST (stale rows in exactly those lanes' pieces;
                // found by the bit-compare test).  LDS operations of one wave execute in issue order: no hardware wait is needed.
                MD_WAVE_LDS_ORDER();
    #pragma unroll
                for (int it = 0; it < 2; ++it) {
                    u32x4 v = *reinterpret_cast<const u32x4 *>(slab + (8 * it + (lane >> 3)) * BN_ES + (lane & 7) * 16);
                    if constexpr (MODE != 2) MD_ADD_BF16X8(v, rres[q2][h * 2 + it], true);
                    MD_BUFFER_STORE_B128(v, rs_y, y_off[h * 2 + it], q * 128, 2);   // (store + guard: device.h)
                }
                MD_WAVE_LDS_ORDER();   // ... and the next half's writes stay behind this half's reads
            }
            BN_STAMP(8 + q2);
        }
    }
#ifdef MD_DIAG
    if (a.dbg && blockIdx.x == (gridDim.x / 2) && tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stp[12] = __builtin_readcyclecounter();
        for (int i = 0; i < 16; ++i) a.dbg[i] = stp[i];
    }
#endif
}

}  // namespace md

using namespace md;

#ifdef MD_DIAG
static unsigned long long *g_bn_stamp_buf = nullptr;
extern "C" int md_diag_set_bn_stamp_buffer(void *p) { g_bn_stamp_buf = (unsigned long long *)p; return MD_OK; }
#endif

// in : x[N,H,W,Cin] bf16 (Cin = 64 or 256), w1[64,Cin] bf16, b12[128] f32 (= b1 | b2), w2[64,576] bf16 (K = tap*64 + ci),
//      w3[256,64] bf16, b3[256] f32, residual[N,H,W,256] bf16 | NULL, wd[256,64] bf16 | NULL, bd[256] f32 | NULL
// out: y[N,H,W,256] bf16
// residual source: wd given (Cin == 64, residual NULL) -> the downsample conv wd . x + bd computed in the launch; residual given ->
// that tensor; neither (Cin == 256) -> x itself.
extern "C" int md_bottleneck(MD_AOT_ARGS) {
    Args g(MD_ARGS, 10, 10);
    g.tensor(0, BF16, 4); g.tensor(1, BF16, 2); g.tensor(2, F32); g.tensor(3, BF16, 2); g.tensor(4, BF16, 2); g.tensor(5, F32);
    g.optional(6, BF16, 4); g.tensor(9, BF16, 4);
    const int64_t N = g.d(0, 0), H = g.d(0, 1), W = g.d(0, 2), Cin = g.d(0, 3);
    g.require((Cin == 64 || Cin == 256) && g.d(1, 0) == 64 && g.d(1, 1) == Cin && g.d(3, 0) == 64 && g.d(3, 1) == 576 &&
              g.d(4, 0) == 256 && g.d(4, 1) == 64 && g.numel(2) == 128 && g.numel(5) >= 256);
    g.require(g.d(9, 0) == N && g.d(9, 1) == H && g.d(9, 2) == W && g.d(9, 3) == 256);
    if (g.given(7)) {   // fused downsample conv
        g.tensor(7, BF16, 2); g.tensor(8, F32);
        g.require(!g.given(6) && g.given(8) && Cin == 64 && g.d(7, 0) == 256 && g.d(7, 1) == 64 && g.numel(8) >= 256);
    } else if (g.given(6)) {
        g.require(g.numel(6) == mul({N, H, W, 256}));
    } else g.require(Cin == 256);
    if (int rc = g.rc()) return rc;
    if (mul({N, H, W}) == 0) return MD_OK;
    if (!g.have({0, 1, 2, 3, 4, 5, 9})) return MD_ERR_ARG;
    if (H > 32000 || W > 32000) return MD_ERR_SIZE;
    const long long x_img = H * W * Cin * 2;
    if (x_img >= 0x7fff0000LL) return MD_ERR_SIZE;
    // 32-bit DMA offsets: run the batch as image chunks whose x tensor stays below 2 GiB (as md_conv2d does; same limit, which
    // tests lower through md_conv_tune.chunk_limit of the call)
    const long long chunk_lim = md_chunk_limit((const md_conv_tune *)extra);
    const long long lim = chunk_lim > x_img ? chunk_lim : x_img;
    const long long per = lim / x_img < N ? lim / x_img : N;
    const int tiles_x = (int)((W + BN_TW - 1) / BN_TW), tiles_y = (int)((H + BN_TH - 1) / BN_TH);
    auto k = params[7] ? bottleneck64_kernel<2> : (params[6] ? bottleneck64_kernel<1> : bottleneck64_kernel<0>);
    int bn_lds = BN_LDS;
#ifdef MD_DIAG
    // occupancy experiment (tools only): MD_BN_LDS > 80 KiB leaves room for ONE workgroup per CU instead of two
    if (const char *e = getenv("MD_BN_LDS")) bn_lds = atoi(e) > BN_LDS ? atoi(e) : BN_LDS;
#endif
    if (ensure_dyn_lds((const void *)k, bn_lds) != MD_OK) return MD_ERR_HIP;
    for (long long n0 = 0; n0 < N; n0 += per) {
        const long long nn = N - n0 < per ? N - n0 : per;
        BottleneckArgs a;
        a.x = (const uint16_t *)params[0] + n0 * H * W * Cin;
        a.w1 = (const uint16_t *)params[1]; a.b1 = (const float *)params[2];
        a.w2 = (const uint16_t *)params[3];
        a.w3 = (const uint16_t *)params[4]; a.b3 = (const float *)params[5];
        a.res = params[7] ? nullptr : (params[6] ? (const uint16_t *)params[6] : (const uint16_t *)params[0]) + n0 * H * W * 256;
        a.wd = (const uint16_t *)params[7]; a.bd = (const float *)params[8];
        a.y = (uint16_t *)params[9] + n0 * H * W * 256;
        a.N = (int)nn; a.H = (int)H; a.W = (int)W; a.Cin = (int)Cin; a.nch = (int)(Cin / 64);
        a.tiles_x = tiles_x; a.tiles_y = tiles_y;
        const long long n_tiles = nn * tiles_x * tiles_y;
        if (n_tiles > 0x7fffffffLL / 8) return MD_ERR_SIZE;
        a.n_tiles = (int)n_tiles;
        a.pt_per_xcd = (a.n_tiles + 7) / 8;
        a.x_bytes = (unsigned)(nn * x_img);
        a.w1_bytes = (unsigned)(64 * Cin * 2);
        a.dbg = nullptr;
#ifdef MD_DIAG
        a.dbg = g_bn_stamp_buf;
#endif
        hipLaunchKernelGGL(k, dim3((unsigned)(a.pt_per_xcd * 8)), dim3(512), bn_lds, (hipStream_t)stream, a);
        md_note_conv_kernel(MD_CONV_KERNEL_BOTTLENECK);
    }
    return launched();
}
