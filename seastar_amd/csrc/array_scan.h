// array_scan.h — the exclusive scan of an array's terms in three dependent
// launches with one tile of kBlock items per block (tile sums, one carry block,
// place): tcp_tx_data.hip's 64-bit scan of the buffers' lengths and its 32-bit
// scan of the cut marks, tcp_ack.hip's scans of the queue entries' lengths and
// of its zero-length marks.
//
// A Load is passed by value in the launch and has
//   V operator()(uint64_t i) const       the term of item i; i is below n
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_launch.h"
#include "wave_scan.h"
#include "wire.h"

namespace array_scan {

using wave_scan::block_inclusive_scan;

constexpr int kBlock = 1024;                 // one item per thread
constexpr int kWaves = kBlock / wave_scan::kWave;
constexpr uint32_t kTile = kBlock;

struct LoadLen {
    const uint32_t* len;
    __device__ __forceinline__ uint64_t operator()(uint64_t i) const { return len[i]; }
};

// The kernels are static: every translation unit that launches one has its own.

template <typename V, typename Load>
static __global__ __launch_bounds__(kBlock) void scan_tile(Load L, uint64_t n, V* __restrict__ tsum) {
    __shared__ V part[kWaves];
    const uint64_t i = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    V total;
    (void)block_inclusive_scan<kWaves>(i < n ? L(i) : V(0), part, &total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// ONE block: the tile sums become exclusive prefixes in place; *closing = the sum.
template <typename V>
static __global__ __launch_bounds__(kBlock) void scan_carry(V* __restrict__ tsum, uint64_t ntiles,
                                                            V* __restrict__ closing) {
    __shared__ V part[kWaves];
    V carry = 0;
    for (uint64_t base = 0; base < ntiles; base += kBlock) {
        const uint64_t t = base + threadIdx.x;
        const V v = t < ntiles ? tsum[t] : V(0);
        V total;
        const V incl = carry + block_inclusive_scan<kWaves>(v, part, &total);
        if (t < ntiles) tsum[t] = incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) *closing = carry;
}

template <typename V, typename Load>
static __global__ __launch_bounds__(kBlock) void scan_place(Load L, uint64_t n, const V* __restrict__ tsum,
                                                            V* __restrict__ out) {
    __shared__ V part[kWaves];
    const uint64_t i = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    const V v = i < n ? L(i) : V(0);
    V total;
    const V incl = block_inclusive_scan<kWaves>(v, part, &total);
    if (i < n) out[i] = tsum[blockIdx.x] + incl - v;
}

// out[0 .. n] = the exclusive scan of L over [0, n) and its sum; `tsum` is one V per tile.
template <typename V, typename Load>
static inline hipError_t scan_array(hipStream_t st, const Load& L, uint64_t n, V* tsum, V* out) {
    const uint64_t ntiles = wire::tiles_of(n, kTile);
    const dim3 tiles(static_cast<unsigned>(ntiles)), block(kBlock);
    host_launch::Chain c{st};
    if (ntiles) c.launch(scan_tile<V, Load>, tiles, block, 0, L, n, tsum);
    c.launch(scan_carry<V>, dim3(1), block, 0, tsum, ntiles, out + n);
    if (ntiles) c.launch(scan_place<V, Load>, tiles, block, 0, L, n, tsum, out);
    return c.e;
}

}  // namespace array_scan
