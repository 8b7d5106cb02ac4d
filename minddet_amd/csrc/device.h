// device.h -- device-side helpers shared by the kernels of libminddet_hip.so: the vector types, the bf16 conversions (the library's one
// rounding rule, the one the float64 judges of tests/*_contract.py model), the packed activations and residual add, the 128-B-row LDS
// swizzle, the gfx950 buffer descriptor and the two ordering / store guards every hot kernel depends on.  Host-side helpers: aot.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Device side: ordering point between LDS writes by SOME lanes of a wave and reads of the same bytes by OTHER lanes of that wave (the
// wave-private transpose slabs of conv_pingpong_kernel<PERS> and bottleneck64_kernel).  To the language these are different threads with no
// synchronisation between them, so hipcc may move -- or, around a divergent `if`, duplicate into the non-writing lanes and run first -- the
// reads across the writes (seen r03: stale rows in exactly those lanes).  A wavefront-scope release / acquire pair orders the memory
// operations, and wave_barrier is a convergent operation: it can be neither duplicated into nor moved across a divergent region.  All
// three lower to no instruction (one wave's LDS operations execute in issue order).  r03 used an empty asm with a memory clobber here,
// which holds only as long as hipcc treats that asm as convergent (r03 ADVICE).
#define MD_WAVE_LDS_ORDER()                                         \
    do {                                                            \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      \
        __builtin_amdgcn_wave_barrier();                            \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");      \
    } while (0)

// Device side: every 128-bit buffer store goes through this macro: the store, then `s_nop 1` in an asm statement that takes the stored value
// as an in / out operand.
// Why (r04, the root cause of r03's "result that was wrong only sometimes"): gfx950 needs two wait states between a VMEM store of more than
// 64 bits and a VALU write of its data registers (the store reads them over several cycles).  hipcc inserts them (`s_nop 1`) -- EXCEPT when
// the store's soffset operand is an SGPR: LLVM's GCNHazardRecognizer::createsVALUHazard exempts that form ("this hazard only exists if the
// instruction is not using a register in the soffset field"), and on this chip the exemption is wrong.  `buffer_store_dwordx4 v[14:17], v84,
// s[8:11], s26 offen` directly followed by `v_lshlrev_b32 v14, 16, v86` stored the NEW v14 in the last four lanes of every 16 -- in some
// tiles of some runs, depending on how long the store waited to issue (profiles/r04_store_data_hazard.txt: reproduced, bisected to one
// not-even-executed branch that changed the schedule, confirmed by two independent fixes).  Any soffset that is not an inline constant is
// exposed: a wave-dependent value, but also a literal above 64, which LLVM materialises in an SGPR.  Whether a build is hit depends only on
// what the scheduler happens to put behind the store -- r03 "fixed" it by rewriting an unrelated expression.
// The guard: the value is live INTO the asm, so its registers cannot be redefined before it, and the asm itself is the two wait states;
// anything the scheduler puts between the store and the asm writes other registers.  No register, 8 bytes of code per store, and it does
// not depend on hipcc's hazard table.  tools/isa_audit.py additionally scans every wide store of every kernel for a VALU write of its
// data registers within two wait states.  V must be a non-const lvalue.
#define MD_BUFFER_STORE_B128(V, RSRC, VOFF, SOFF, AUX)                                   \
    do {                                                                                 \
        __builtin_amdgcn_raw_buffer_store_b128((V), (RSRC), (int)(VOFF), (SOFF), (AUX)); \
        asm volatile("s_nop 1" : "+v"(V));                                               \
    } while (0)

namespace md {

// LDS accesses use these BUILTIN vector types only: hipcc's waitcnt pass puts s_waitcnt vmcnt(0) in front of an LDS access without type-based
// alias info (HIP's float4 / uint2 structs) while LDS-DMAs are pending -- r02: that drained the W2-tap / W3 DMAs of bottleneck64_kernel in
// front of the T1 / T2 epilogues instead of letting the epilogue math run under their latency
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;   // the A / B fragment of the f16 MFMAs (ppreader.hip)
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

// ---- bf16 <-> fp32.  A bf16 value travels as the low 16 bits of an integer (bf2f shifts any higher bits out).
__device__ __forceinline__ float bf2f(unsigned v16) { return __uint_as_float(v16 << 16); }
// one packed word (two bf16) -> its two values, low half first
__device__ __forceinline__ f32x2 bf2f_pair(unsigned w) { return (f32x2){__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)}; }
// round-to-nearest-even; NaN stays NaN (quiet)
__device__ __forceinline__ uint16_t f2bf(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// the same rounding without the NaN branch.  Precondition: f is finite (a NaN whose payload sits in the low 16 bits only would round
// to infinity); the grouped conv's and the pillar encoder's epilogues, whose inputs are finite by construction
__device__ __forceinline__ uint16_t f2bf_finite(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// two fp32 -> packed bf16 (round-to-nearest-even) in ONE instruction (gfx950 v_cvt_pk_bf16_f32).  r01 stamps: the software
// rounding (9 VALU per value, 64 values per lane) made the epilogue VALU-bound at four workgroups per CU.
__device__ __forceinline__ unsigned pk_bf16(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

// ---- activations
__device__ __forceinline__ unsigned pk_relu_bf16(unsigned v) {  // max(x, 0) on a packed bf16 pair: as signed 16-bit integers
    unsigned r;
    asm("v_pk_max_i16 %0, %1, 0" : "=v"(r) : "v"(v));
    return r;
}
// SiLU with the hardware reciprocal (v_rcp_f32, 1 ulp) instead of an IEEE division (v_div_scale / fmas / fixup: ~10 VALU per
// value, 64 values per lane in an epilogue that is VALU-bound at four workgroups per CU); the result is rounded to bf16.
__device__ __forceinline__ float silu(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }
// the sigmoid of the decode kernels: IEEE division and expf, not the fast forms above (scores are compared against thresholds)
__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- residual add: V = bf16(V + RES) on eight bf16 values (V an lvalue, RES a value, both u32x4: v_pk_add_f32 + one pack per pair), then
// the packed ReLU where RELU holds (evaluated per pair).  A macro and not a function: with this loop's body behind a call, even a
// forceinline one, hipcc allocates the registers of the conv.hip kernels around it differently (same instructions, ~500 fewer moves in one
// build, and nothing promises the next build that); the text below is the loop as every epilogue wrote it out.
// Two words at a time (the epilogues that add before the LDS transpose): bf2f_pair(a) + bf2f_pair(b), then pk_bf16.
#define MD_ADD_BF16X8(V, RES, RELU)                                                                                                \
    do {                                                                                                                           \
        const md::u32x4 res__ = (RES);                                                                                             \
        _Pragma("unroll") for (int k__ = 0; k__ < 4; ++k__) {                                                                      \
            const md::f32x2 sum__ = (md::f32x2){__uint_as_float((V)[k__] << 16), __uint_as_float((V)[k__] & 0xffff0000u)} +        \
                                    (md::f32x2){__uint_as_float(res__[k__] << 16), __uint_as_float(res__[k__] & 0xffff0000u)};     \
            (V)[k__] = md::pk_bf16(sum__.x, sum__.y);                                                                              \
            if (RELU) (V)[k__] = md::pk_relu_bf16((V)[k__]);                                                                       \
        }                                                                                                                          \
    } while (0)

// byte offset of 16-B chunk `chunk` of row `row` in an LDS tile of 128-B rows ([row][64 k] bf16): the chunk index is XOR-swizzled by
// (row >> 1) & 7, on the DMA's SOURCE chunk and on the ds_read_b128 fragment reads alike (conflict free)
__device__ __forceinline__ int swz128(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// Buffer descriptor (V#) over `bytes` bytes at p: stride 0 (raw buffer: the offset is a byte offset, checked against `bytes`, so an
// out-of-range load returns 0 and an out-of-range store is dropped).  The flag word is descriptor word 3, whose layout is the chip's:
// on gfx950 DATA_FORMAT (bits 18:15) = 4 = BUF_DATA_FORMAT_32, a valid format as raw accesses need one, and every other field zero
// (NUM_FORMAT, the DST_SEL swizzles, index stride, add-tid).  A kernel never spells the literal: a port changes it here.
constexpr int kSrdFlagsGfx950 = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t srd(const void *p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, bytes, kSrdFlagsGfx950);
}

}  // namespace md
