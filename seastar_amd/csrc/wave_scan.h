// wave_scan.h — a lane's index and the inclusive scan across a 64-lane wave,
// for steer.hip (32-bit counts) and send.hip (64-bit frames << 32 | bytes).
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

}  // namespace wave_scan
