// wave_scan.h — a lane's index and the inclusive scan across a 64-lane wave
// and across a block of whole waves: of sums (steer.hip, udp.hip, eth.hip and
// tcp.hip's 32-bit counts, send.hip's 64-bit frames << 32 | bytes, reasm.hip's
// both) and of any associative op (reasm.hip's and tcp_data.hip's segmented
// scans).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace wave_scan {

constexpr int kWave = 64;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & (kWave - 1); }

// A struct that is scanned brings an overload of its own next to its
// definition, member by member.
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

// The same scans of any associative op; op(a, b): a is the earlier one.
template <typename T, typename Op>
__device__ __forceinline__ T wave_inclusive_scan(T v, Op op) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T o = shfl_up(v, d);
        if (lane_id() >= static_cast<uint32_t>(d)) v = op(o, v);
    }
    return v;
}

// Every thread folds the aggregates of the waves before its own, as
// block_inclusive_scan does.
template <int kWaves, typename T, typename Op>
__device__ __forceinline__ T block_scan_serial(T v, const T& ident, T* part, T* total, Op op) {
    const uint32_t wave = threadIdx.x / kWave;
    v = wave_inclusive_scan(v, op);
    __syncthreads();  // the last call's readers are done with part
    if (lane_id() == kWave - 1) part[wave] = v;
    __syncthreads();
    T before = ident, all = ident;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const T p = part[w];
        if (static_cast<uint32_t>(w) < wave) before = op(before, p);
        all = op(all, p);
    }
    *total = all;
    return op(before, v);
}

// The waves' aggregates scanned in place by the first kWaves lanes of the
// first wave: one barrier more, and a thread reads two values of `part`, not
// kWaves, and combines once, not kWaves times.  tcp_data.hip's scans, whose
// elements are costly to combine, use this form and reasm.hip's the other;
// neither layer has been measured with the other's form.
template <int kWaves, typename T, typename Op>
__device__ __forceinline__ T block_scan(T v, const T& ident, T* part, T* total, Op op) {
    const uint32_t wave = threadIdx.x / kWave;
    v = wave_inclusive_scan(v, op);
    __syncthreads();  // the last call's readers are done with part
    if (lane_id() == kWave - 1) part[wave] = v;
    __syncthreads();
    if (wave == 0) {
        T p = lane_id() < kWaves ? part[lane_id()] : ident;
#pragma unroll
        for (int d = 1; d < kWaves; d <<= 1) {
            const T o = shfl_up(p, d);
            if (lane_id() >= static_cast<uint32_t>(d)) p = op(o, p);
        }
        if (lane_id() < kWaves) part[lane_id()] = p;
    }
    __syncthreads();
    *total = part[kWaves - 1];
    return wave ? op(part[wave - 1], v) : v;
}

}  // namespace wave_scan
