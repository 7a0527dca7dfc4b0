// wave_scan.h — a lane's index, the inclusive scan across a 64-lane wave and
// across a block of whole waves, for steer.hip (32-bit counts), send.hip
// (64-bit frames << 32 | bytes) and reasm.hip (both).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace wave_scan {

constexpr int kWave = 64;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & (kWave - 1); }

__device__ __forceinline__ uint32_t shfl_up(uint32_t v, int d) { return __shfl_up(v, d, kWave); }
__device__ __forceinline__ uint64_t shfl_up(uint64_t v, int d) {
    return __shfl_up(static_cast<unsigned long long>(v), d, kWave);
}

template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T o = shfl_up(v, d);
        if (lane_id() >= static_cast<uint32_t>(d)) v += o;
    }
    return v;
}

// Inclusive scan over the threads of a block of kWaves waves; *total = the
// block's sum.  `part` is LDS for one value per wave; the call may be repeated.
template <int kWaves, typename T>
__device__ __forceinline__ T block_inclusive_scan(T v, T* part, T* total) {
    const uint32_t wave = threadIdx.x / kWave;
    const T incl = wave_inclusive_scan(v);
    __syncthreads();  // the last call's readers are done with part
    if (lane_id() == kWave - 1) part[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const T p = part[w];
        if (static_cast<uint32_t>(w) < wave) before += p;
        all += p;
    }
    *total = all;
    return before + incl;
}

}  // namespace wave_scan
