// compact.h — the stable compaction of the items of a batch that pass a
// predicate, in three dependent launches with one tile of kBlock items per
// block: reasm.hip's fragment records (FrameRecord) and eth.hip's ARP learn
// candidates (Candidate).
//
// A predicate is passed by value in the launch and has
//   Record                               what an accepted item becomes
//   Out                                  the element type of the output array
//   bool operator()(uint64_t i, Record*) is item i accepted (false past the batch)
//   static void store(Out*, uint64_t pos, const Record&)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_launch.h"
#include "wave_scan.h"

namespace compact {

using wave_scan::block_inclusive_scan;
using wave_scan::kWave;

// The kernels are static: every translation unit that launches one has its own.

template <int kBlock, typename Pred>
static __global__ __launch_bounds__(kBlock) void tile_kernel(Pred P, uint32_t* __restrict__ tcount) {
    __shared__ uint32_t part[kBlock / kWave];
    typename Pred::Record r;
    const uint32_t a = P(uint64_t(blockIdx.x) * kBlock + threadIdx.x, &r) ? 1u : 0u;
    uint32_t total;
    (void)block_inclusive_scan<kBlock / kWave>(a, part, &total);
    if (threadIdx.x == 0) tcount[blockIdx.x] = total;
}

// ONE block: the per-tile sums become inclusive prefixes in place; *d_count = the sum.
template <int kBlock>
static __global__ __launch_bounds__(kBlock) void carry_kernel(uint32_t* __restrict__ tcount, uint64_t ntiles,
                                                              uint32_t* __restrict__ d_count) {
    __shared__ uint32_t part[kBlock / kWave];
    uint32_t carry = 0;
    for (uint64_t base = 0; base < ntiles; base += kBlock) {
        const uint64_t t = base + threadIdx.x;
        const uint32_t v = t < ntiles ? tcount[t] : 0u;
        uint32_t total;
        const uint32_t incl = carry + block_inclusive_scan<kBlock / kWave>(v, part, &total);
        if (t < ntiles) tcount[t] = incl;
        carry += total;
    }
    if (threadIdx.x == 0) *d_count = carry;
}

template <int kBlock, typename Pred>
static __global__ __launch_bounds__(kBlock) void place_kernel(Pred P, const uint32_t* __restrict__ tcount,
                                                              typename Pred::Out* __restrict__ d_out) {
    __shared__ uint32_t part[kBlock / kWave];
    typename Pred::Record r;
    const bool ok = P(uint64_t(blockIdx.x) * kBlock + threadIdx.x, &r);
    uint32_t total;
    const uint32_t incl = block_inclusive_scan<kBlock / kWave>(ok ? 1u : 0u, part, &total);
    const uint32_t base = blockIdx.x ? tcount[blockIdx.x - 1] : 0u;
    if (ok) Pred::store(d_out, uint64_t(base) + incl - 1u, r);
}

// The three launches over ntiles tiles; `tcount` is workspace, one word per
// tile.  Without a tile only the carry kernel runs, for *d_count = 0.
template <int kBlock, typename Pred>
static inline hipError_t run(hipStream_t st, const Pred& P, uint64_t ntiles, uint32_t* tcount, uint32_t* d_count,
                             typename Pred::Out* d_out) {
    const dim3 tiles(static_cast<unsigned>(ntiles)), block(kBlock);
    host_launch::Chain c{st};
    if (ntiles) c.launch(tile_kernel<kBlock, Pred>, tiles, block, 0, P, tcount);
    c.launch(carry_kernel<kBlock>, dim3(1), block, 0, tcount, ntiles, d_count);
    if (ntiles) c.launch(place_kernel<kBlock, Pred>, tiles, block, 0, P, tcount, d_out);
    return c.e;
}

}  // namespace compact
