// bucket_pass.h — the stable count / scan / scatter pass over an 8-bit bucket
// that steer.hip (the shard of a packet), eth.hip (the protocol of a frame),
// udp.hip (the channel of a datagram) and the radix sorts of tcp.hip and
// reasm.hip (one digit of a key) are built from:
//   count    one block per tile: hist_clear / hist_add / hist_store leave the
//            tile's per-bucket counts in column blockIdx.x of ws[bucket][pitch]
//   scan     scan_buckets: per bucket an exclusive scan over the tiles in place
//            and the bucket bases -> d_first; a radix pass launches
//            scan_rows_kernel alone and lets its scatter scan the 256 totals
//   scatter  one block per tile: bucket_base or digit_base, then TileRank:
//            an item's place is its bucket's base + its offset inside the tile
// The callers keep their loads, decode, stores and barriers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "host_launch.h"
#include "wave_scan.h"

namespace bucket_pass {

using wave_scan::block_inclusive_scan;
using wave_scan::kWave;
using wave_scan::lane_id;
using wave_scan::wave_inclusive_scan;

constexpr uint32_t kDigits = 256;          // the buckets of a radix pass
constexpr uint32_t kScanOneBlockMax = 32;  // buckets the one-block scan takes (two rows per wave of 1024 threads)

// A row of ws holds one count per tile, padded to whole 16-byte loads.
template <typename T>
__host__ __device__ inline T pitch_of(T ntiles) { return (ntiles + 3u) & ~T(3); }

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

// ---------------------------------------------------------------- count

template <int kBuckets>
__device__ __forceinline__ void hist_clear(uint32_t (&hist)[kBuckets]) {
    if (threadIdx.x < kBuckets) hist[threadIdx.x] = 0;
}

// One LDS add per distinct bucket of the wave: only a count comes out.
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t b, bool valid) {
    const uint64_t m = match_bucket(b, valid);
    if (valid && (m & lanes_below()) == 0) atomicAdd(&hist[b], static_cast<uint32_t>(__popcll(m)));
}

__device__ __forceinline__ void hist_store(const uint32_t* hist, uint32_t buckets, uint32_t* __restrict__ ws,
                                           uint32_t pitch) {
    if (threadIdx.x < buckets) ws[uint64_t(threadIdx.x) * pitch + blockIdx.x] = hist[threadIdx.x];
}

// ---------------------------------------------------------------- scan

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

// One wave: the bucket totals scanned into d_first (buckets + 1 entries).
__device__ __forceinline__ void scan_totals(const uint32_t* total, uint32_t buckets, uint32_t* __restrict__ d_first) {
    const uint32_t lane = lane_id();
    uint32_t carry = 0;
    for (uint32_t base = 0; base < buckets; base += kWave) {
        const uint32_t b = base + lane;
        const uint32_t c = b < buckets ? total[b] : 0u;
        const uint32_t incl = wave_inclusive_scan(c);
        if (b < buckets) d_first[b] = carry + incl - c;
        carry += __shfl(incl, kWave - 1, kWave);
    }
    if (lane == 0) d_first[buckets] = carry;
}

// The kernels are static templates: a translation unit has its own copy of
// those it launches and none of the others.

// Few buckets (at most kScanOneBlockMax), or no tile at all: ONE block does
// both, wave w taking the rows of buckets w, w + kBlock / 64, ...
template <int kBlock, int kMaxBuckets>
static __global__ __launch_bounds__(kBlock) void scan_kernel(uint32_t* __restrict__ ws, uint32_t ntiles, uint32_t pitch,
                                                             uint32_t buckets, uint32_t* __restrict__ d_first) {
    __shared__ uint32_t total[kMaxBuckets];
    const uint32_t wave = threadIdx.x / kWave;
    for (uint32_t b = wave; b < buckets; b += kBlock / kWave) {
        const uint32_t sum = scan_row(ws, b, ntiles, pitch);
        if (lane_id() == 0) total[b] = sum;
    }
    __syncthreads();
    if (wave == 0) scan_totals(total, buckets, d_first);
}

// Many buckets: one block (one wave) per bucket scans its row and leaves the
// total behind the rows; a second launch of one wave scans the totals.  One
// compute unit alone takes 24 us for the 257 rows of 512 tiles of a
// 1 Mi-packet batch at 255 shards, whether or not its loads are batched
// (DESIGN.md §5.12): the rows are spread over the device instead.
template <int kBlock = kWave>
static __global__ __launch_bounds__(kBlock) void scan_rows_kernel(uint32_t* __restrict__ ws, uint32_t ntiles,
                                                                  uint32_t pitch, uint32_t* __restrict__ totals) {
    static_assert(kBlock == kWave, "one wave per row");
    const uint32_t sum = scan_row(ws, blockIdx.x, ntiles, pitch);
    if (lane_id() == 0) totals[blockIdx.x] = sum;
}

template <int kBlock = kWave>
static __global__ __launch_bounds__(kBlock) void scan_totals_kernel(const uint32_t* __restrict__ totals,
                                                                    uint32_t buckets, uint32_t* __restrict__ d_first) {
    static_assert(kBlock == kWave, "one wave");
    scan_totals(totals, buckets, d_first);
}

// The scan step of a pass over `buckets` buckets: ws[bucket][pitch] becomes
// per-bucket exclusive prefixes over the tiles, d_first the bucket bases.  The
// many-bucket path leaves the bucket totals in `totals`, which a caller of at
// most kScanOneBlockMax buckets need not have.
template <int kBlock, int kMaxBuckets>
static inline hipError_t scan_buckets(hipStream_t st, uint32_t* ws, uint32_t ntiles, uint32_t pitch, uint32_t buckets,
                                      uint32_t* d_first, uint32_t* totals) {
    host_launch::Chain c{st};
    if constexpr (kMaxBuckets > kScanOneBlockMax) {
        if (buckets > kScanOneBlockMax && ntiles != 0) {
            c.launch(scan_rows_kernel<>, dim3(buckets), dim3(kWave), 0, ws, ntiles, pitch, totals);
            c.launch(scan_totals_kernel<>, dim3(1), dim3(kWave), 0, totals, buckets, d_first);
            return c.e;
        }
    }
    c.launch(scan_kernel<kBlock, kMaxBuckets>, dim3(1), dim3(kBlock), 0, ws, ntiles, pitch, buckets, d_first);
    return c.e;
}

// ---------------------------------------------------------------- scatter

// base[bucket]: where the tile's items of the bucket start in the grouped arrays.
__device__ __forceinline__ void bucket_base(uint32_t* base, uint32_t buckets, const uint32_t* __restrict__ d_first,
                                            const uint32_t* __restrict__ ws, uint32_t pitch) {
    if (threadIdx.x < buckets) base[threadIdx.x] = d_first[threadIdx.x] + ws[uint64_t(threadIdx.x) * pitch + blockIdx.x];
}

// The same for a radix pass, whose bases are the exclusive scan of the 256
// digit totals, one digit per thread.  `part`: LDS, one value per wave.
template <int kWaves>
__device__ __forceinline__ void digit_base(uint32_t* base, const uint32_t* __restrict__ totals,
                                           const uint32_t* __restrict__ counts, uint32_t pitch, uint32_t* part) {
    const uint32_t t = threadIdx.x < kDigits ? totals[threadIdx.x] : 0u;
    uint32_t all;
    const uint32_t incl = block_inclusive_scan<kWaves>(t, part, &all);
    if (threadIdx.x < kDigits) base[threadIdx.x] = incl - t + counts[uint64_t(threadIdx.x) * pitch + blockIdx.x];
}

// An item's offset inside its tile among the items of its bucket, for a tile of
// kRounds rounds of kWaves waves: round r holds the tile's items
// [64 kWaves r, 64 kWaves (r + 1)), one per thread.  cnt[slot][bucket] is the
// number of items of the bucket in (round, wave) pair `slot`, then their offset
// inside the tile: 32 bits for the one-round tile, 16 for a tile of several
// rounds, whose LDS that halves.
//   clear(buckets); barrier; mark(r, b, valid) for every round; barrier;
//   scan(buckets); barrier; offset(r, b) for every valid item
template <int kWaves, int kRounds, int kBuckets>
struct TileRank {
    static constexpr int kSlots = kRounds * kWaves;
    static constexpr int kBlock = kWaves * kWave;
    using Count = std::conditional_t<kRounds == 1, uint32_t, uint16_t>;
    static_assert(kRounds == 1 || kRounds * kBlock <= 0xFFFF, "an offset inside the tile fits the count");

    Count (*cnt)[kBuckets];
    uint32_t rank[kRounds];  // the item's peers of its bucket in the lanes below

    __device__ __forceinline__ TileRank() {
        __shared__ Count lds[kSlots][kBuckets];
        cnt = lds;
    }

    __device__ __forceinline__ void clear(uint32_t buckets) {
        if constexpr (kRounds == 1) {
            for (uint32_t k = threadIdx.x; k < kSlots * kBuckets; k += kBlock) (&cnt[0][0])[k] = 0;
        } else if (threadIdx.x < buckets) {
#pragma unroll
            for (int s = 0; s < kSlots; ++s) cnt[s][threadIdx.x] = 0;
        }
    }

    __device__ __forceinline__ void mark(int r, uint32_t b, bool valid) {
        const uint64_t m = match_bucket(b, valid);
        rank[r] = static_cast<uint32_t>(__popcll(m & lanes_below()));
        if (valid && rank[r] == 0) cnt[r * kWaves + threadIdx.x / kWave][b] = static_cast<Count>(__popcll(m));
    }

    // Per bucket the serial exclusive scan over the slots, in item order.
    __device__ __forceinline__ void scan(uint32_t buckets) {
        if (threadIdx.x < buckets) {
            uint32_t run = 0;
#pragma unroll
            for (int s = 0; s < kSlots; ++s) {
                const uint32_t c = cnt[s][threadIdx.x];
                cnt[s][threadIdx.x] = static_cast<Count>(run);
                run += c;
            }
        }
    }

    __device__ __forceinline__ uint32_t offset(int r, uint32_t b) const {
        return cnt[r * kWaves + threadIdx.x / kWave][b] + rank[r];
    }
};

}  // namespace bucket_pass
