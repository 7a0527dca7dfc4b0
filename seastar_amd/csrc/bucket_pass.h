// bucket_pass.h — the pieces of a stable count / scan / scatter pass over an
// 8-bit bucket that steer.hip (the shard of a packet) and reasm.hip (one digit
// of a radix sort) share: a lane's peers of the same bucket inside its wave,
// and the in-place exclusive scan of one bucket's row of per-tile counts.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "wave_scan.h"

namespace bucket_pass {

using wave_scan::kWave;
using wave_scan::lane_id;
using wave_scan::wave_inclusive_scan;

// The lanes of the wave whose bucket equals this lane's, among the valid ones:
// eight ballots, one per bit of the 8-bit bucket.
__device__ __forceinline__ uint64_t match_bucket(uint32_t b, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const uint64_t set = __ballot((b >> bit) & 1u);
        m &= ((b >> bit) & 1u) ? set : ~set;
    }
    return m;
}

__device__ __forceinline__ uint64_t lanes_below() { return (uint64_t(1) << lane_id()) - 1u; }

// One wave scans one bucket's row of per-tile counts in place (exclusive): each
// lane takes four consecutive tiles (one 16-byte load), the lanes' sums are
// scanned across the wave, 256 tiles at a time with the sum carried along.
// Returns the row's total (the same in every lane).
__device__ __forceinline__ uint32_t scan_row(uint32_t* __restrict__ ws, uint32_t b, uint32_t ntiles,
                                             uint32_t tile_pitch) {
    uint4* const row = reinterpret_cast<uint4*>(ws + uint64_t(b) * tile_pitch);
    const uint32_t lane = lane_id();
    uint32_t carry = 0;
    for (uint32_t base = 0; base < ntiles; base += kWave * 4) {
        const uint32_t t = base + lane * 4;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (t < ntiles) v = row[t / 4];
        if (t + 1 >= ntiles) v.y = 0;  // the row's padding up to tile_pitch
        if (t + 2 >= ntiles) v.z = 0;
        if (t + 3 >= ntiles) v.w = 0;
        const uint32_t sum = v.x + v.y + v.z + v.w;
        const uint32_t incl = wave_inclusive_scan(sum);
        const uint32_t ex = carry + incl - sum;
        if (t < ntiles) row[t / 4] = make_uint4(ex, ex + v.x, ex + v.x + v.y, ex + v.x + v.y + v.z);
        carry += __shfl(incl, kWave - 1, kWave);
    }
    return carry;
}

}  // namespace bucket_pass
