// workgroup.h -- the integer wave and workgroup primitives of the kernels, stated once: the 64-lane scan, the workgroup exclusive scan, the
// one-workgroup scan over block counts, the block sum, ballot ranks and the in-order append, and the pieces of the three-pass stable
// compaction built on them.  Device code only.  No LDS of its own: every function that needs some takes it from the caller, and says
// which barriers it holds -- every lane of the workgroup calls those.  Integers only: the float and double reductions stay where their
// summation order is documented (loss_common.h block_sums and the kernels' own).
#pragma once
#include <hip/hip_runtime.h>

namespace md {

// ---------------------------------------------------------------------------------------------------- one wave
// inclusive prefix sum over the 64 lanes (int or unsigned)
template <typename T> __device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
// the sum over the 64 lanes, in every lane (int or unsigned)
template <typename T> __device__ __forceinline__ T wave_sum_all(T v) {
    static_assert(T(1) / T(2) == T(0), "integers only: a float sum's order belongs to its kernel");
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// set bits of a ballot below this lane: the lane's place among the wave's voters
__device__ __forceinline__ int lane_rank(unsigned long long ballot) {
    const int lane = threadIdx.x & 63;
    return __popcll(ballot & ((1ull << lane) - 1ull));
}

// ---------------------------------------------------------------------------------------------------- one workgroup
// exclusive prefix sum of one value per lane over a workgroup of WAVES waves; total: the workgroup's sum, in every lane.
// wsum: WAVES values of LDS.  Two barriers, the first before wsum is written: an earlier call's readers are done with it.
template <int WAVES, typename T> __device__ __forceinline__ T block_exclusive_scan(T v, T *wsum, T &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = wave_inclusive_scan(v);
    __syncthreads();
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    total = all;
    return before + inc - v;
}
// one workgroup of WAVES waves: bsum[0 .. nb) becomes its exclusive prefix in place, 64 WAVES counts at a time with a carry; returns the
// total, in every lane.  wsum as above
template <int WAVES> __device__ __forceinline__ int scan_block_counts(int *bsum, int nb, int *wsum) {
    int carry = 0;
    for (int base = 0; base < nb; base += 64 * WAVES) {
        const int k = base + threadIdx.x;
        const int v = k < nb ? bsum[k] : 0;
        int all;
        const int ex = block_exclusive_scan<WAVES>(v, wsum, all);
        if (k < nb) bsum[k] = carry + ex;
        carry += all;
    }
    return carry;
}
// a block sum of integers (256 lanes; red: 4 ints); every lane gets the sum
__device__ __forceinline__ int block_count(int v, int *red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();   // red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
// in-order append: the slot of a lane that keeps its element, *count slots being taken before the workgroup's first (read behind the
// barrier).  Leaves the waves' numbers of kept elements in wave_cnt (the caller advances its count by their sum).  One barrier
__device__ __forceinline__ int block_append(bool keep, int *wave_cnt, const int *count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    int at = *count;
    for (int w = 0; w < wave; ++w) at += wave_cnt[w];
    return at + lane_rank(bal);
}

// ---------------------------------------------------------------------------------------------------- stable compaction
// 256 rows per workgroup.  Pass 1: block_keep_count leaves the workgroup's number of kept rows in bsum[block].  Pass 2 (one workgroup of
// 256): compaction_offsets turns bsum[0 .. nb) into its exclusive prefix in place, the total in bsum[nb].  Pass 3: block_rank is a kept
// row's place in the output.  wcnt, wsum: 4 ints of LDS; all three hold barriers.
__device__ __forceinline__ void block_keep_count(bool keep, int *wcnt, int *bsum) {
    const unsigned long long bal = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}
__device__ __forceinline__ void compaction_offsets(int *bsum, int nb, int *wsum) {
    const int total = scan_block_counts<4>(bsum, nb, wsum);
    if (threadIdx.x == 0) bsum[nb] = total;
    __syncthreads();
}
__device__ __forceinline__ int block_rank(bool keep, int *wcnt, const int *bsum) { return block_append(keep, wcnt, bsum + blockIdx.x); }

}  // namespace md
