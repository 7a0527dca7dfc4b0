// reasm.hip — IPv4 reassembly for a batch on the GPU: the fragment records of
// a frames batch, and the merge of the records into fragment-list datagrams
// (sccsum.h, "Rx reassembly").
//
// What it restates from the reference (paths relative to the reference tree):
//   ipv4::handle_received_packet   src/net/ip.cc:159-220 (destination, the branch at 164)
//   ipv4::frag::merge / is_complete   src/net/ip.cc:412-437
//   packet_merger::merge           include/seastar/net/packet-util.hh:45-151
//   ipv4_frag_id                   include/seastar/net/ip.hh:243-256
//
// No payload byte moves: a reassembled datagram is one sccsum_gather_desc per
// fragment.  Only PLAIN keys are decided here (no empty piece, no overlap, at
// most one MF-clear record and that one last in offset order): for them the
// reference's outcome does not depend on arrival order.  Every other key goes
// to the host bucket whole, where the reference's own order-dependent rules
// (packet-util.hh:55-86) are replayed.
//
// Plain dependent launches on the caller's stream, no block ever waiting on
// another one and no atomic deciding a position (the only atomics are LDS adds
// into a histogram and LDS minima, whose results do not depend on their order):
//   records:  compact.h's tile / carry / place over FrameRecord   stable compaction of the accepted frames
//   reasm:    key                 (mix32(key) << 13 | offset / 8) per record
//             6 x sort_count / bucket_pass's scan_rows / sort_scatter   stable LSD radix sort, 8-bit digits
//             detect              head / tail of a group (equal mix), neighbour tests
//             seg_tile / seg_carry / seg_place   segmented scan over the sorted order:
//                                 a group's flags, its latest arrival, its head
//             classify            per record: complete / pending / host, who completes
//             dg_tile / dg_carry / dg_place   datagrams in completion order, the
//                                 capacity prefix, the per-datagram outputs
//             emit                one descriptor per record of an emitted datagram
//             st_tile / st_carry / st_place   stable compaction of the pending and host records
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "bucket_pass.h"
#include "compact.h"
#include "host_launch.h"
#include "sccsum.h"
#include "sccsum_diag.h"
#include "wave_scan.h"
#include "wire.h"

namespace reasm {

using bucket_pass::kDigits;
using bucket_pass::scan_rows_kernel;
using host_launch::Chain;
using host_launch::misaligned;
using host_launch::stream_ok;
using host_launch::Workspace;
using wave_scan::block_inclusive_scan;
using wire::be32_at;
using wire::fmix32;
using wire::pseudo_seed;
using wire::tiles_of;

constexpr int kWave = 64;
constexpr int kSortBlock = 256;            // threads of the sort's count / scatter kernels
constexpr int kSortWaves = kSortBlock / kWave;
constexpr int kSortRounds = 8;              // records per thread: round r of a tile is its records [256 r, 256 r + 256)
constexpr uint32_t kSortTile = kSortBlock * kSortRounds;
constexpr int kScanBlock = 1024;            // threads of the scan kernels: one record each
constexpr int kScanWaves = kScanBlock / kWave;
constexpr uint32_t kScanTile = kScanBlock;
constexpr int kFlatBlock = 256;             // threads of the kernels that need no neighbour's result
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kMaxRecords = 0x7FFFFFFFull;
constexpr int kOffBits = 13;                // the fragment offset in 8-byte units
constexpr int kPasses = 6;                  // 13 + 32 bits in digits of 8, 5, 8, 8, 8, 8
constexpr int kPassShift[kPasses] = {0, 8, 13, 21, 29, 37};
constexpr uint32_t kPassMask[kPasses] = {0xFF, 0x1F, 0xFF, 0xFF, 0xFF, 0xFF};

// flags of a record at its sorted position
constexpr uint32_t kHead = 1u;    // first of its group
constexpr uint32_t kTail = 2u;    // last of its group
constexpr uint32_t kMixed = 4u;   // its key differs from its predecessor's: two keys share the mix
constexpr uint32_t kBad = 8u;     // not plain: empty, overlaps its predecessor, or follows an MF-clear record
constexpr uint32_t kGap = 16u;    // does not touch its predecessor / a head not at offset 0
constexpr uint32_t kOpen = 32u;   // a tail with MF set: the last fragment is missing

// The 32-bit mix of an ipv4_frag_id the sort groups by.  For one (src, dst)
// pair it is a bijection of (id, proto); distinct keys that collide differ in
// an address.
__host__ __device__ inline uint32_t key_mix(uint32_t src, uint32_t dst, uint32_t id, uint32_t proto) {
    uint32_t h = fmix32(src + 0x9E3779B9u);
    h = fmix32(h ^ dst);
    return fmix32(h + ((id << 8) | proto) * 0x9E3779B1u);
}

// A record as four 64-bit words (sccsum_frag_rec, 32 bytes, 8-byte aligned).
struct Rec {
    uint64_t frame, addr, w2, w3;
    __device__ uint32_t src() const { return static_cast<uint32_t>(addr); }
    __device__ uint32_t dst() const { return static_cast<uint32_t>(addr >> 32); }
    __device__ uint32_t id() const { return static_cast<uint32_t>(w2 & 0xFFFFu); }
    __device__ uint32_t proto() const { return static_cast<uint32_t>((w2 >> 16) & 0xFFu); }
    __device__ uint32_t mf() const { return static_cast<uint32_t>((w2 >> 24) & 0xFFu); }
    __device__ uint32_t offset() const { return static_cast<uint32_t>((w2 >> 32) & 0xFFFFu); }
    __device__ uint32_t hdr_len() const { return static_cast<uint32_t>(w2 >> 48); }
    __device__ uint32_t len() const { return static_cast<uint32_t>(w3 & 0xFFFFu); }
    __device__ uint32_t end() const { return offset() + len(); }
    __device__ bool same_key(const Rec& o) const { return addr == o.addr && ((w2 ^ o.w2) & 0xFFFFFFu) == 0; }
};

__device__ __forceinline__ Rec load_rec(const sccsum_frag_rec* __restrict__ rec, uint64_t i) {
    const uint64_t* const w = reinterpret_cast<const uint64_t*>(rec + i);
    return Rec{w[0], w[1], w[2], w[3]};
}

__device__ __forceinline__ void store_rec(sccsum_frag_rec* __restrict__ rec, uint64_t i, const Rec& r) {
    uint64_t* const w = reinterpret_cast<uint64_t*>(rec + i);
    w[0] = r.frame;
    w[1] = r.addr;
    w[2] = r.w2;
    w[3] = r.w3;
}

// ---------------------------------------------------------------- records

// compact.h's predicate: frame i's record when it is accepted.  The caller's
// status masks, then the tests of ip.cc:128-144 again on the header itself (a
// frame the masks let through is still never read outside the buffer), then
// the destination (ip.cc:159-162).
struct FrameRecord {
    const uint8_t* bytes;
    uint64_t bytes_len;
    const uint64_t* off;
    const uint32_t* len;
    const uint8_t* status;
    uint64_t n;
    uint32_t need, reject, host, tag;

    using Record = Rec;
    using Out = sccsum_frag_rec;

    __device__ __forceinline__ bool operator()(uint64_t i, Rec* out) const {
        if (i >= n) return false;
        if (!wire::status_passes(status[i], need, reject)) return false;
        wire::Ipv4View ip;
        const bool trusted = wire::ipv4_view(bytes, bytes_len, off[i], len[i], &ip);
        const uint32_t frag = ip.frag;
        const uint32_t offset = (frag & 0x1FFFu) << 3;
        // `|`: one branch for both tests, so that the fragment word's load is not sunk behind the first
        // one (a memory round trip: 74 -> 93 us for the records of 1 Mi fragments)
        if (!trusted | (offset + ip.ip_len > 65535u)) return false;
        const uint32_t dst = ip.dst();
        if (host != 0 && dst != host) return false;
        out->frame = reinterpret_cast<uint64_t>(ip.h);
        out->addr = uint64_t(ip.src()) | (uint64_t(dst) << 32);
        out->w2 = uint64_t(ip.id()) | (uint64_t(ip.proto()) << 16) | (uint64_t((frag >> 13) & 1u) << 24) |
                  (uint64_t(offset) << 32) | (uint64_t(ip.hdr_len) << 48);
        out->w3 = uint64_t(ip.ip_len - ip.hdr_len) | (uint64_t(tag) << 32);
        return true;
    }

    static __device__ __forceinline__ void store(Out* __restrict__ d_rec, uint64_t pos, const Rec& r) {
        store_rec(d_rec, pos, r);
    }
};

// ---------------------------------------------------------------- sort

__global__ __launch_bounds__(kFlatBlock) void key_kernel(const sccsum_frag_rec* __restrict__ rec, uint32_t m,
                                                         uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * kFlatBlock + threadIdx.x;
    if (i >= m) return;
    const Rec r = load_rec(rec, i);
    key[i] = (uint64_t(key_mix(r.src(), r.dst(), r.id(), r.proto())) << kOffBits) | (r.offset() >> 3);
    idx[i] = i;
}

// A tile's keys (all loads issued before any use) as digits.
__device__ __forceinline__ void tile_digits(const uint64_t* __restrict__ key, uint32_t m, uint32_t first, int shift,
                                            uint32_t mask, uint64_t (&k)[kSortRounds], uint32_t (&d)[kSortRounds]) {
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        const uint32_t i = first + r * kSortBlock + threadIdx.x;
        k[r] = i < m ? key[i] : 0u;
    }
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) d[r] = static_cast<uint32_t>(k[r] >> shift) & mask;
}

__global__ __launch_bounds__(kSortBlock) void sort_count_kernel(const uint64_t* __restrict__ key, uint32_t m, int shift,
                                                                uint32_t mask, uint32_t* __restrict__ counts,
                                                                uint32_t pitch) {
    __shared__ uint32_t hist[kDigits];
    bucket_pass::hist_clear(hist);
    __syncthreads();
    const uint32_t first = blockIdx.x * kSortTile;
    uint64_t k[kSortRounds];
    uint32_t d[kSortRounds];
    tile_digits(key, m, first, shift, mask, k, d);
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) bucket_pass::hist_add(hist, d[r], first + r * kSortBlock + threadIdx.x < m);
    __syncthreads();
    bucket_pass::hist_store(hist, kDigits, counts, pitch);
}

__global__ __launch_bounds__(kSortBlock) void sort_scatter_kernel(const uint64_t* __restrict__ key,
                                                                  const uint32_t* __restrict__ idx, uint32_t m, int shift,
                                                                  uint32_t mask, const uint32_t* __restrict__ counts,
                                                                  uint32_t pitch, const uint32_t* __restrict__ totals,
                                                                  uint64_t* __restrict__ key_out,
                                                                  uint32_t* __restrict__ idx_out) {
    // base[digit]: where the tile's records of the digit start
    __shared__ uint32_t base[kDigits];
    __shared__ uint32_t part[kSortWaves];
    bucket_pass::TileRank<kSortWaves, kSortRounds, kDigits> rank;
    bucket_pass::digit_base<kSortWaves>(base, totals, counts, pitch, part);
    rank.clear(kDigits);
    __syncthreads();
    const uint32_t first = blockIdx.x * kSortTile;
    uint64_t k[kSortRounds];
    uint32_t d[kSortRounds];
    uint32_t src[kSortRounds];
    tile_digits(key, m, first, shift, mask, k, d);
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        const uint32_t i = first + r * kSortBlock + threadIdx.x;
        src[r] = i < m ? idx[i] : 0u;
    }
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) rank.mark(r, d[r], first + r * kSortBlock + threadIdx.x < m);
    __syncthreads();
    rank.scan(kDigits);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        const uint32_t i = first + r * kSortBlock + threadIdx.x;
        if (i < m) {
            const uint32_t pos = base[d[r]] + rank.offset(r, d[r]);
            if (pos < m) {  // always true: the counts are this pass's own
                key_out[pos] = k[r];
                idx_out[pos] = src[r];
            }
        }
    }
}

// ---------------------------------------------------------------- groups

// Sorted position j: its group is the run of equal mix; inside it the records
// lie in offset order, ties in arrival order.
__global__ __launch_bounds__(kFlatBlock) void detect_kernel(const sccsum_frag_rec* __restrict__ rec,
                                                            const uint64_t* __restrict__ key,
                                                            const uint32_t* __restrict__ idx, uint32_t m,
                                                            uint32_t* __restrict__ flags) {
    const uint32_t j = blockIdx.x * kFlatBlock + threadIdx.x;
    if (j >= m) return;
    const uint64_t mix = key[j] >> kOffBits;
    const bool head = j == 0 || (key[j - 1] >> kOffBits) != mix;
    const bool tail = j + 1 == m || (key[j + 1] >> kOffBits) != mix;
    const Rec r = load_rec(rec, idx[j]);
    uint32_t f = (head ? kHead : 0u) | (tail ? kTail : 0u);
    if (r.len() == 0) f |= kBad;
    if (head) {
        if (r.offset() != 0) f |= kGap;
    } else {
        const Rec p = load_rec(rec, idx[j - 1]);
        if (!p.same_key(r)) f |= kMixed;
        if (p.mf() == 0 || p.end() > r.offset()) f |= kBad;
        if (p.end() != r.offset()) f |= kGap;
    }
    if (tail && r.mf() != 0) f |= kOpen;
    flags[j] = f;
}

// What a segmented scan carries: hp = 1 + the position of the latest head in
// the span (0: none), and over the records since that head (or over the whole
// span) the OR of their flags and the latest arrival index.
struct Seg {
    uint32_t hp, fl, arr;
};

__device__ __forceinline__ Seg seg_join(const Seg& a, const Seg& b) {  // a before b
    if (b.hp) return b;
    return Seg{a.hp, a.fl | b.fl, a.arr > b.arr ? a.arr : b.arr};
}

__device__ __forceinline__ Seg shfl_up(const Seg& v, int d) {
    return Seg{wave_scan::shfl_up(v.hp, d), wave_scan::shfl_up(v.fl, d), wave_scan::shfl_up(v.arr, d)};
}

// Inclusive segmented scan over the 1024 threads of a block; *total = the block's.
__device__ __forceinline__ Seg seg_block_scan(Seg v, Seg* part, Seg* total) {
    return wave_scan::block_scan_serial<kScanWaves>(
        v, Seg{0, 0, 0}, part, total, [](const Seg& a, const Seg& b) { return seg_join(a, b); });
}

__device__ __forceinline__ Seg seg_of(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ idx, uint32_t m,
                                      uint32_t j) {
    if (j >= m) return Seg{0, 0, 0};
    const uint32_t f = flags[j];
    return Seg{(f & kHead) ? j + 1 : 0u, f & ~(kHead | kTail), idx[j]};
}

__global__ __launch_bounds__(kScanBlock) void seg_tile_kernel(const uint32_t* __restrict__ flags,
                                                              const uint32_t* __restrict__ idx, uint32_t m,
                                                              uint32_t* __restrict__ segt) {
    __shared__ Seg part[kScanWaves];
    Seg total;
    (void)seg_block_scan(seg_of(flags, idx, m, blockIdx.x * kScanTile + threadIdx.x), part, &total);
    if (threadIdx.x == 0) {
        segt[3 * blockIdx.x] = total.hp;
        segt[3 * blockIdx.x + 1] = total.fl;
        segt[3 * blockIdx.x + 2] = total.arr;
    }
}

// ONE block: the tiles' values become inclusive prefixes in place.
__global__ __launch_bounds__(kScanBlock) void seg_carry_kernel(uint32_t* __restrict__ segt, uint32_t ntiles) {
    __shared__ Seg part[kScanWaves];
    Seg carry{0, 0, 0};
    for (uint32_t base = 0; base < ntiles; base += kScanBlock) {
        const uint32_t t = base + threadIdx.x;
        Seg v{0, 0, 0};
        if (t < ntiles) v = Seg{segt[3 * t], segt[3 * t + 1], segt[3 * t + 2]};
        Seg total;
        const Seg incl = seg_join(carry, seg_block_scan(v, part, &total));
        if (t < ntiles) {
            segt[3 * t] = incl.hp;
            segt[3 * t + 1] = incl.fl;
            segt[3 * t + 2] = incl.arr;
        }
        carry = seg_join(carry, total);
    }
}

constexpr uint32_t kStComplete = SCCSUM_REASM_COMPLETE;
constexpr uint32_t kStPending = SCCSUM_REASM_PENDING;
constexpr uint32_t kStHost = SCCSUM_REASM_HOST;

// What a group's records share, stored at the group's head position by its tail.
struct Groups {
    uint32_t* state;  // complete / pending / host
    uint32_t* arr;    // the latest arrival index among its records
    uint32_t* end;    // the tail's offset + len: E of a complete key
    uint32_t* cnt;    // its records
};

__global__ __launch_bounds__(kScanBlock) void seg_place_kernel(const sccsum_frag_rec* __restrict__ rec,
                                                               const uint32_t* __restrict__ flags,
                                                               const uint32_t* __restrict__ idx, uint32_t m,
                                                               const uint32_t* __restrict__ segt,
                                                               uint32_t* __restrict__ gh, Groups G) {
    __shared__ Seg part[kScanWaves];
    const uint32_t j = blockIdx.x * kScanTile + threadIdx.x;
    Seg total;
    Seg v = seg_block_scan(seg_of(flags, idx, m, j), part, &total);
    if (blockIdx.x) {
        const uint32_t t = blockIdx.x - 1;
        v = seg_join(Seg{segt[3 * t], segt[3 * t + 1], segt[3 * t + 2]}, v);
    }
    if (j >= m || v.hp == 0) return;  // position 0 is a head: hp >= 1
    const uint32_t g = v.hp - 1;
    gh[j] = g;
    if (flags[j] & kTail) {
        G.state[g] = (v.fl & (kMixed | kBad)) ? kStHost : (v.fl & (kGap | kOpen)) ? kStPending : kStComplete;
        G.arr[g] = v.arr;
        G.end[g] = load_rec(rec, idx[j]).end();
        G.cnt[g] = j - g + 1;
    }
}

// Per record, at its arrival index: its group's state and head, and for the
// record that completes a key (the last of them to arrive) the datagram's
// descriptor count and length.
__global__ __launch_bounds__(kFlatBlock) void classify_kernel(const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ gh, Groups G, uint32_t m,
                                                              uint8_t* __restrict__ state0, uint32_t* __restrict__ gha,
                                                              uint32_t* __restrict__ c_cnt,
                                                              uint32_t* __restrict__ c_len) {
    const uint32_t j = blockIdx.x * kFlatBlock + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = idx[j];
    const uint32_t g = gh[j];
    if (i >= m || g >= m) return;  // never: idx is a permutation, g a position
    const uint32_t st = G.state[g];
    const bool completes = st == kStComplete && G.arr[g] == i;
    state0[i] = static_cast<uint8_t>(st);
    gha[i] = g;
    c_cnt[i] = completes ? G.cnt[g] : 0u;
    c_len[i] = completes ? G.end[g] : 0u;
}

// ---------------------------------------------------------------- datagrams

// Record i as a datagram: count << 32 | descriptors, and its bytes.
__device__ __forceinline__ void dgram_of(const uint32_t* __restrict__ c_cnt, const uint32_t* __restrict__ c_len,
                                         uint32_t m, uint32_t i, uint64_t* cd, uint64_t* by) {
    const uint32_t c = i < m ? c_cnt[i] : 0u;
    *cd = c ? (uint64_t(1) << 32) | c : 0u;
    *by = c ? c_len[i] : 0u;
}

__global__ __launch_bounds__(kScanBlock) void dg_tile_kernel(const uint32_t* __restrict__ c_cnt,
                                                             const uint32_t* __restrict__ c_len, uint32_t m,
                                                             uint64_t* __restrict__ t1) {
    __shared__ uint64_t part[kScanWaves];
    uint64_t cd, by, tcd, tby;
    dgram_of(c_cnt, c_len, m, blockIdx.x * kScanTile + threadIdx.x, &cd, &by);
    (void)block_inclusive_scan<kScanWaves>(cd, part, &tcd);
    (void)block_inclusive_scan<kScanWaves>(by, part, &tby);
    if (threadIdx.x == 0) {
        t1[2 * uint64_t(blockIdx.x)] = tcd;
        t1[2 * uint64_t(blockIdx.x) + 1] = tby;
    }
}

// ONE block: inclusive prefixes over the tiles in place, then the capacity
// prefix: the layout bytes only grow, so the datagrams that fit are a prefix;
// the tile the cap falls in is scanned again for the first that does not.
__global__ __launch_bounds__(kScanBlock) void dg_carry_kernel(const uint32_t* __restrict__ c_cnt,
                                                              const uint32_t* __restrict__ c_len, uint32_t m,
                                                              uint64_t* __restrict__ t1, uint32_t ntiles,
                                                              uint64_t max_out_bytes, uint64_t* __restrict__ head,
                                                              uint64_t* __restrict__ d_total,
                                                              uint32_t* __restrict__ d_dgram_first) {
    __shared__ uint64_t part[kScanWaves];
    __shared__ unsigned int cut_tile, cut_slot;
    __shared__ uint64_t at_cut;
    if (threadIdx.x == 0) {
        cut_tile = kNone;
        cut_slot = kScanTile;
    }
    __syncthreads();
    uint64_t ccd = 0, cby = 0;
    for (uint32_t base = 0; base < ntiles; base += kScanBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint64_t cd = t < ntiles ? t1[2 * uint64_t(t)] : 0u;
        const uint64_t by = t < ntiles ? t1[2 * uint64_t(t) + 1] : 0u;
        uint64_t tcd, tby;
        const uint64_t icd = ccd + block_inclusive_scan<kScanWaves>(cd, part, &tcd);
        const uint64_t iby = cby + block_inclusive_scan<kScanWaves>(by, part, &tby);
        if (t < ntiles) {
            t1[2 * uint64_t(t)] = icd;
            t1[2 * uint64_t(t) + 1] = iby;
            if (iby > max_out_bytes) atomicMin(&cut_tile, t);
        }
        ccd += tcd;
        cby += tby;
    }
    __syncthreads();
    const uint32_t tc = cut_tile;
    uint64_t emitted = ccd;
    if (tc != kNone) {
        const uint64_t bcd = tc ? t1[2 * uint64_t(tc - 1)] : 0u;
        const uint64_t bby = tc ? t1[2 * uint64_t(tc - 1) + 1] : 0u;
        uint64_t cd, by, tcd, tby;
        dgram_of(c_cnt, c_len, m, tc * kScanTile + threadIdx.x, &cd, &by);
        const uint64_t icd = block_inclusive_scan<kScanWaves>(cd, part, &tcd);
        const uint64_t iby = block_inclusive_scan<kScanWaves>(by, part, &tby);
        if (bby + iby > max_out_bytes) atomicMin(&cut_slot, threadIdx.x);
        __syncthreads();
        if (threadIdx.x == cut_slot) at_cut = bcd + icd - cd;  // cut_slot < kScanTile: the tile's total does not fit
        __syncthreads();
        emitted = at_cut;
    }
    if (threadIdx.x == 0) {
        const uint64_t dgrams = emitted >> 32, descs = emitted & 0xFFFFFFFFu;
        head[0] = dgrams;
        d_total[0] = dgrams;
        d_total[1] = descs;
        d_dgram_first[dgrams] = static_cast<uint32_t>(descs);  // the closing entry
    }
}

struct Rss {
    uint32_t* hash;  // per-datagram output (nullptr: no key given)
    uint32_t w[96];  // the 32 key bits starting at key bit j (toeplitz.hh:78-98)
};

__device__ __forceinline__ uint32_t toeplitz96(const Rss& P, uint32_t d0, uint32_t d1, uint32_t d2) {
    uint32_t h = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        h ^= (d0 & (0x80000000u >> j)) ? P.w[j] : 0u;
        h ^= (d1 & (0x80000000u >> j)) ? P.w[32 + j] : 0u;
        h ^= (d2 & (0x80000000u >> j)) ? P.w[64 + j] : 0u;
    }
    return h;
}

struct Dgrams {
    uint32_t* first;
    uint64_t* off;
    uint32_t* len;
    uint32_t* seed;
    uint32_t* head;
    uint32_t* last;
};

__global__ __launch_bounds__(kScanBlock) void dg_place_kernel(const sccsum_frag_rec* __restrict__ rec,
                                                              const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ c_cnt,
                                                              const uint32_t* __restrict__ c_len,
                                                              const uint32_t* __restrict__ gha, uint32_t m,
                                                              const uint64_t* __restrict__ t1,
                                                              const uint64_t* __restrict__ head,
                                                              uint32_t* __restrict__ dnum, Dgrams D, Rss R) {
    __shared__ uint64_t part[kScanWaves];
    const uint32_t i = blockIdx.x * kScanTile + threadIdx.x;
    uint64_t cd, by, tcd, tby;
    dgram_of(c_cnt, c_len, m, i, &cd, &by);
    uint64_t xcd = block_inclusive_scan<kScanWaves>(cd, part, &tcd) - cd;
    uint64_t xby = block_inclusive_scan<kScanWaves>(by, part, &tby) - by;
    if (blockIdx.x) {
        xcd += t1[2 * uint64_t(blockIdx.x - 1)];
        xby += t1[2 * uint64_t(blockIdx.x - 1) + 1];
    }
    if (i >= m) return;
    const uint64_t d = xcd >> 32;
    const bool emitted = cd != 0 && d < head[0];
    dnum[i] = emitted ? static_cast<uint32_t>(d) : kNone;
    if (!emitted) return;
    const uint32_t hi = idx[gha[i]];  // the offset-0 record: its header is the one frag::merge keeps
    const Rec h = load_rec(rec, hi);
    const uint32_t E = static_cast<uint32_t>(by);
    const uint32_t proto = h.proto();
    D.first[d] = static_cast<uint32_t>(xcd);
    D.off[d] = xby;
    D.len[d] = E;
    D.seed[d] = (proto == 6 || proto == 17) ? pseudo_seed(h.src(), h.dst(), proto, E & 0xFFFFu) : 0u;
    D.head[d] = hi;
    D.last[d] = i;
    if (R.hash) {
        // ip.cc:186-197: src, dst, then the ports when the datagram holds the TCP / UDP header.  Every
        // fragment but the last is a multiple of 8 bytes long, so the four bytes lie in the head record.
        const uint32_t need = proto == 6 ? 20u : proto == 17 ? 8u : 0u;
        uint32_t ports = 0;
        if (need && E >= need) ports = be32_at(reinterpret_cast<const uint8_t*>(h.frame) + h.hdr_len());
        R.hash[d] = toeplitz96(R, h.src(), h.dst(), ports);
    }
}

__global__ __launch_bounds__(kFlatBlock) void emit_kernel(const sccsum_frag_rec* __restrict__ rec,
                                                          const uint32_t* __restrict__ idx,
                                                          const uint32_t* __restrict__ gh, Groups G,
                                                          const uint32_t* __restrict__ dnum, uint32_t m,
                                                          const uint32_t* __restrict__ d_dgram_first,
                                                          const uint64_t* __restrict__ d_dgram_off,
                                                          sccsum_gather_desc* __restrict__ d_desc) {
    const uint32_t j = blockIdx.x * kFlatBlock + threadIdx.x;
    if (j >= m) return;
    const uint32_t g = gh[j];
    if (G.state[g] != kStComplete) return;
    const uint32_t d = dnum[G.arr[g]];
    if (d == kNone) return;  // past the capacity prefix: pending
    const Rec r = load_rec(rec, idx[j]);
    const uint64_t k = uint64_t(d_dgram_first[d]) + (j - g);
    if (k >= m) return;  // never: a datagram's descriptors are its group's records
    uint64_t* const out = reinterpret_cast<uint64_t*>(d_desc + k);
    out[0] = r.frame + r.hdr_len();
    out[1] = uint64_t(static_cast<uint32_t>(d_dgram_off[d] + r.offset())) | (uint64_t(r.len()) << 32);
}

// ---------------------------------------------------------------- pending / host

struct Final {
    const uint8_t* state0;
    const uint32_t* gha;
    const uint32_t* garr;
    const uint32_t* dnum;
    uint32_t m;
};

// Record i's final state: a complete key past the capacity prefix is pending.
__device__ __forceinline__ uint32_t final_state(const Final& F, uint32_t i) {
    if (i >= F.m) return 0;
    const uint32_t st = F.state0[i];
    if (st == kStComplete && F.dnum[F.garr[F.gha[i]]] == kNone) return kStPending;
    return st;
}

__device__ __forceinline__ uint64_t ph_of(uint32_t st) {  // pending << 32 | host
    return st == kStPending ? uint64_t(1) << 32 : st == kStHost ? 1u : 0u;
}

__global__ __launch_bounds__(kScanBlock) void st_tile_kernel(Final F, uint64_t* __restrict__ t2) {
    __shared__ uint64_t part[kScanWaves];
    uint64_t total;
    (void)block_inclusive_scan<kScanWaves>(ph_of(final_state(F, blockIdx.x * kScanTile + threadIdx.x)), part, &total);
    if (threadIdx.x == 0) t2[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanBlock) void st_carry_kernel(uint64_t* __restrict__ t2, uint32_t ntiles,
                                                              uint64_t* __restrict__ d_total) {
    __shared__ uint64_t part[kScanWaves];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < ntiles; base += kScanBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint64_t v = t < ntiles ? t2[t] : 0u;
        uint64_t total;
        const uint64_t incl = carry + block_inclusive_scan<kScanWaves>(v, part, &total);
        if (t < ntiles) t2[t] = incl;
        carry += total;
    }
    if (threadIdx.x == 0) {
        d_total[2] = carry >> 32;
        d_total[3] = carry & 0xFFFFFFFFu;
    }
}

__global__ __launch_bounds__(kScanBlock) void st_place_kernel(const sccsum_frag_rec* __restrict__ rec, Final F,
                                                              const uint64_t* __restrict__ t2,
                                                              sccsum_frag_rec* __restrict__ d_pending,
                                                              sccsum_frag_rec* __restrict__ d_host,
                                                              uint8_t* __restrict__ d_rec_state) {
    __shared__ uint64_t part[kScanWaves];
    const uint32_t i = blockIdx.x * kScanTile + threadIdx.x;
    const uint32_t st = final_state(F, i);
    const uint64_t v = ph_of(st);
    uint64_t total;
    uint64_t x = block_inclusive_scan<kScanWaves>(v, part, &total) - v;
    if (blockIdx.x) x += t2[blockIdx.x - 1];
    if (i >= F.m) return;
    d_rec_state[i] = static_cast<uint8_t>(st);
    if (st == kStPending) store_rec(d_pending, x >> 32, load_rec(rec, i));
    if (st == kStHost) store_rec(d_host, x & 0xFFFFFFFFu, load_rec(rec, i));
}

// m == 0: the totals and the closing CSR entry.
__global__ void empty_kernel(uint64_t* __restrict__ d_total, uint32_t* __restrict__ d_dgram_first) {
    if (threadIdx.x < 4) d_total[threadIdx.x] = 0;
    if (threadIdx.x == 0) d_dgram_first[0] = 0;
}

// ---------------------------------------------------------------- host side

static_assert(sizeof(sccsum_frag_rec) == 32 && offsetof(sccsum_frag_rec, src) == 8 &&
                  offsetof(sccsum_frag_rec, id) == 16 && offsetof(sccsum_frag_rec, proto) == 18 &&
                  offsetof(sccsum_frag_rec, mf) == 19 && offsetof(sccsum_frag_rec, offset) == 20 &&
                  offsetof(sccsum_frag_rec, hdr_len) == 22 && offsetof(sccsum_frag_rec, len) == 24 &&
                  offsetof(sccsum_frag_rec, tag) == 28,
              "the kernels read a record as four 64-bit words");
static_assert(sizeof(sccsum_gather_desc) == 16 && offsetof(sccsum_gather_desc, dst_off) == 8 &&
                  offsetof(sccsum_gather_desc, len) == 12,
              "the emit kernel stores a descriptor as two 64-bit words");

// The workspace of a run over m records, every array on a 16-byte boundary.
struct Layout {
    uint64_t key[2], idx[2], counts, totals, flags, gh, gstate, garr, gend, gcnt, segt, state0, gha, ccnt, clen, dnum,
        t1, t2, head, bytes;
    uint32_t sort_tiles, pitch, scan_tiles;
};

Layout layout(uint64_t m) {
    Layout L{};
    host_launch::Carver c;
    L.sort_tiles = static_cast<uint32_t>(tiles_of(m, kSortTile));
    L.pitch = bucket_pass::pitch_of(L.sort_tiles);
    L.scan_tiles = static_cast<uint32_t>(tiles_of(m, kScanTile));
    L.head = c.take(16, 16);
    for (int k = 0; k < 2; ++k) L.key[k] = c.take(8 * m, 16);
    for (int k = 0; k < 2; ++k) L.idx[k] = c.take(4 * m, 16);
    L.counts = c.take(uint64_t(kDigits) * L.pitch * 4, 16);
    L.totals = c.take(kDigits * 4, 16);
    L.flags = c.take(4 * m, 16);
    L.gh = c.take(4 * m, 16);
    L.gstate = c.take(4 * m, 16);
    L.garr = c.take(4 * m, 16);
    L.gend = c.take(4 * m, 16);
    L.gcnt = c.take(4 * m, 16);
    L.segt = c.take(12 * uint64_t(L.scan_tiles), 16);
    L.state0 = c.take(m, 16);
    L.gha = c.take(4 * m, 16);
    L.ccnt = c.take(4 * m, 16);
    L.clen = c.take(4 * m, 16);
    L.dnum = c.take(4 * m, 16);
    L.t1 = c.take(16 * uint64_t(L.scan_tiles), 16);
    L.t2 = c.take(8 * uint64_t(L.scan_tiles), 16);
    L.bytes = c.end();
    return L;
}

}  // namespace reasm

extern "C" {

int sccsum_reasm_sort_tile_records(void) { return static_cast<int>(reasm::kSortTile); }
int sccsum_reasm_scan_tile_records(void) { return static_cast<int>(reasm::kScanTile); }

uint32_t sccsum_reasm_key_mix(uint32_t src_host, uint32_t dst_host, uint16_t id, uint8_t proto) {
    return reasm::key_mix(src_host, dst_host, id, proto);
}

uint64_t sccsum_ipv4_reasm_workspace(uint64_t m) {
    return reasm::layout(m > reasm::kMaxRecords ? reasm::kMaxRecords : m).bytes;
}

int sccsum_ipv4_frag_records(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                             const uint8_t* d_status, uint32_t need, uint32_t reject, uint64_t n,
                             uint32_t host_address, uint32_t tag, sccsum_frag_rec* d_rec, uint32_t* d_count,
                             void* d_workspace, void* stream) {
    using namespace reasm;
    if (n > kMaxRecords || (need | reject) > 0xFFu) return SCCSUM_EINVAL;
    if (!d_count || !d_workspace || misaligned(d_count, 4) || misaligned(d_workspace, 16)) return SCCSUM_EINVAL;
    if (n != 0) {
        if ((!d_bytes && bytes_len != 0) || !d_off || !d_len || !d_status || !d_rec) return SCCSUM_EINVAL;
        if (misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_rec, 8)) return SCCSUM_EINVAL;
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, -1);
    if (rc != SCCSUM_OK) return rc;
    const FrameRecord F{static_cast<const uint8_t*>(d_bytes), bytes_len, d_off, d_len, d_status, n, need, reject,
                        host_address, tag};
    return static_cast<int>(compact::run<kScanBlock>(st, F, tiles_of(n, kScanTile), static_cast<uint32_t*>(d_workspace),
                                                     d_count, d_rec));
}

int sccsum_ipv4_reasm(const sccsum_frag_rec* d_rec, uint64_t m, uint64_t max_out_bytes, const uint8_t* key,
                      uint32_t key_len, const sccsum_reasm_out* out, void* d_workspace, void* stream) {
    using namespace reasm;
    if (!out || m > kMaxRecords || max_out_bytes > 0xFFFFFFFFull) return SCCSUM_EINVAL;
    if (!out->d_total || !out->d_dgram_first || misaligned(out->d_total, 8) || misaligned(out->d_dgram_first, 4)) {
        return SCCSUM_EINVAL;
    }
    if ((key != nullptr) != (out->d_dgram_hash != nullptr) || (key && key_len < 4) || (!key && key_len != 0)) {
        return SCCSUM_EINVAL;
    }
    if (misaligned(d_workspace, 16)) return SCCSUM_EINVAL;
    if (m != 0) {
        if (!d_rec || !d_workspace || !out->d_desc || !out->d_dgram_off || !out->d_dgram_len || !out->d_dgram_seed ||
            !out->d_dgram_head || !out->d_dgram_last || !out->d_pending || !out->d_host || !out->d_rec_state) {
            return SCCSUM_EINVAL;
        }
        if (misaligned(d_rec, 8) || misaligned(out->d_desc, 8) || misaligned(out->d_dgram_off, 8) ||
            misaligned(out->d_dgram_len, 4) || misaligned(out->d_dgram_seed, 4) || misaligned(out->d_dgram_head, 4) ||
            misaligned(out->d_dgram_last, 4) || misaligned(out->d_dgram_hash, 4) || misaligned(out->d_pending, 8) ||
            misaligned(out->d_host, 8)) {
            return SCCSUM_EINVAL;
        }
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, -1);
    if (rc != SCCSUM_OK) return rc;
    Chain c{st};
    if (m == 0) {
        c.launch(empty_kernel, dim3(1), dim3(kWave), 0, out->d_total, out->d_dgram_first);
        return c.rc();
    }

    const Layout L = layout(m);
    const Workspace ws(d_workspace);
    const uint32_t n = static_cast<uint32_t>(m);
    const dim3 flat(static_cast<unsigned>(tiles_of(m, kFlatBlock))), sort(L.sort_tiles), scan(L.scan_tiles);
    const dim3 flat_block(kFlatBlock), sort_block(kSortBlock), scan_block(kScanBlock);

    c.launch(key_kernel, flat, flat_block, 0, d_rec, n, ws.u64(L.key[0]), ws.u32(L.idx[0]));
    for (int p = 0; p < kPasses; ++p) {  // an even number of passes: the sorted order ends in key[0] / idx[0]
        const uint64_t* const kin = ws.u64(L.key[p & 1]);
        const uint32_t* const iin = ws.u32(L.idx[p & 1]);
        c.launch(sort_count_kernel, sort, sort_block, 0, kin, n, kPassShift[p], kPassMask[p], ws.u32(L.counts),
                 L.pitch);
        c.launch(scan_rows_kernel<>, dim3(kDigits), dim3(kWave), 0, ws.u32(L.counts), L.sort_tiles, L.pitch,
                 ws.u32(L.totals));
        c.launch(sort_scatter_kernel, sort, sort_block, 0, kin, iin, n, kPassShift[p], kPassMask[p], ws.u32(L.counts),
                 L.pitch, ws.u32(L.totals), ws.u64(L.key[(p + 1) & 1]), ws.u32(L.idx[(p + 1) & 1]));
    }
    static_assert(kPasses % 2 == 0, "the sorted order must end where it started");
    const uint64_t* const skey = ws.u64(L.key[0]);
    const uint32_t* const sidx = ws.u32(L.idx[0]);
    const Groups G{ws.u32(L.gstate), ws.u32(L.garr), ws.u32(L.gend), ws.u32(L.gcnt)};
    c.launch(detect_kernel, flat, flat_block, 0, d_rec, skey, sidx, n, ws.u32(L.flags));
    c.launch(seg_tile_kernel, scan, scan_block, 0, ws.u32(L.flags), sidx, n, ws.u32(L.segt));
    c.launch(seg_carry_kernel, dim3(1), scan_block, 0, ws.u32(L.segt), L.scan_tiles);
    c.launch(seg_place_kernel, scan, scan_block, 0, d_rec, ws.u32(L.flags), sidx, n, ws.u32(L.segt), ws.u32(L.gh), G);
    c.launch(classify_kernel, flat, flat_block, 0, sidx, ws.u32(L.gh), G, n, ws.at<uint8_t>(L.state0), ws.u32(L.gha),
             ws.u32(L.ccnt), ws.u32(L.clen));
    const uint32_t* const ccnt = ws.u32(L.ccnt);
    const uint32_t* const clen = ws.u32(L.clen);
    c.launch(dg_tile_kernel, scan, scan_block, 0, ccnt, clen, n, ws.u64(L.t1));
    c.launch(dg_carry_kernel, dim3(1), scan_block, 0, ccnt, clen, n, ws.u64(L.t1), L.scan_tiles, max_out_bytes,
             ws.u64(L.head), out->d_total, out->d_dgram_first);
    Rss R{};
    R.hash = out->d_dgram_hash;
    if (key) {
        // w[j] = the 32 key bits starting at bit j (MSB first), bits past key_len zero
        auto bit = [&](uint32_t k) -> uint32_t {
            return k < 8u * key_len ? (key[k >> 3] >> (7u - (k & 7u))) & 1u : 0u;
        };
        for (uint32_t j = 0; j < 96; ++j) {
            uint32_t w = 0;
            for (uint32_t t = 0; t < 32; ++t) w |= bit(j + t) << (31u - t);
            R.w[j] = w;
        }
    }
    const Dgrams D{out->d_dgram_first, out->d_dgram_off, out->d_dgram_len,
                   out->d_dgram_seed,  out->d_dgram_head, out->d_dgram_last};
    c.launch(dg_place_kernel, scan, scan_block, 0, d_rec, sidx, ccnt, clen, ws.u32(L.gha), n, ws.u64(L.t1),
             ws.u64(L.head), ws.u32(L.dnum), D, R);
    c.launch(emit_kernel, flat, flat_block, 0, d_rec, sidx, ws.u32(L.gh), G, ws.u32(L.dnum), n, out->d_dgram_first,
             out->d_dgram_off, out->d_desc);
    const Final F{ws.at<uint8_t>(L.state0), ws.u32(L.gha), ws.u32(L.garr), ws.u32(L.dnum), n};
    c.launch(st_tile_kernel, scan, scan_block, 0, F, ws.u64(L.t2));
    c.launch(st_carry_kernel, dim3(1), scan_block, 0, ws.u64(L.t2), L.scan_tiles, out->d_total);
    c.launch(st_place_kernel, scan, scan_block, 0, d_rec, F, ws.u64(L.t2), out->d_pending, out->d_host,
             out->d_rec_state);
    return c.rc();
}

}  // extern "C"
