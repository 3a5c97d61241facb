// mpf_reduce.h - the deterministic reductions of the loss, metric and statistics kernels (device only)
//
// "The same bits on every run" means every addition happens in an order the code fixes, never in the order the hardware schedules.  The three steps
// below are that order; a kernel that needs a workgroup or grid sum includes them instead of writing them again:
//   wave    xor butterfly over the 64 lanes, offsets 32, 16, ..., 1: every lane ends with the result
//   block   lane 0 of each wave parks its sum in LDS; after the barrier the wave slots are added in the order wave 0, 1, ..., WAVES - 1
//   grid    a one-workgroup finish kernel: thread t gathers partials t, t + THREADS, ... (the caller's loop - layouts differ), then a halving tree
//
// PRECONDITION of everything here: EVERY lane of the wave (mpf_wave_*) or thread of the workgroup (mpf_block_*) must make the call.  A butterfly
// reads its partner lane's register, and a lane that has left hands over nothing defined.  Kernels therefore keep the threads past the end of their
// data alive with the neutral value (0 for a sum, the empty range for min / max) and never `return` before the reduction.
#pragma once
#include <hip/hip_runtime.h>

// float, double, int, unsigned
template <typename T>
__device__ __forceinline__ T mpf_wave_sum(T v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// integers; float goes through fmaxf / fminf below and drops a NaN as they do
template <typename T>
__device__ __forceinline__ T mpf_wave_max(T v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const T o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

template <typename T>
__device__ __forceinline__ T mpf_wave_min(T v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const T o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ float mpf_wave_max(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

__device__ __forceinline__ float mpf_wave_min(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}

// The workgroup's sums of part[0 .. nq) -> dst[0 .. nq), written by threads 0 .. nq - 1.  lds: WAVES * NQ values of the calling kernel's LDS.
// There is no barrier after the slots are read: a caller that uses lds again synchronises first.
template <int WAVES, int NQ, typename T>
__device__ __forceinline__ void mpf_block_sums(const T (&part)[NQ], int nq, T *lds, T *dst)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = 0; q < nq; ++q) {
        const T v = mpf_wave_sum(part[q]);
        if (lane == 0) lds[wave * NQ + q] = v;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)nq) {
        T v = lds[threadIdx.x];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += lds[w * NQ + threadIdx.x];
        dst[threadIdx.x] = v;
    }
}

// The finish kernel's tree over its THREADS threads' gathered values; sR: THREADS doubles of LDS.  The sum is in sR[0] when the call returns; a
// caller that runs the tree again synchronises after reading it.
template <int THREADS>
__device__ __forceinline__ void mpf_block_tree_sum(double v, double *sR)
{
    sR[threadIdx.x] = v;
    __syncthreads();
    for (int m = THREADS / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) sR[threadIdx.x] += sR[threadIdx.x + m];
        __syncthreads();
    }
}
