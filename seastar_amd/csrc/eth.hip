// eth.hip — the Ethernet layer around the IPv4 path on the GPU: rx demux by
// eth_proto with the 14-byte trim, the ARP learn candidates of an IPv4 bucket,
// and on tx the next-hop lookup plus the Ethernet header in front of every
// frame's fragment list (sccsum.h, "Link layer").
//
// What it restates from the reference (paths relative to the reference tree):
//   interface::dispatch_packet   src/net/net.cc:324-357
//   _arp.learn(from, h.src_ip)   src/net/ip.cc:147-149, include/seastar/net/arp.hh:247-248
//   ipv4::get_l2_dst_address     src/net/ip.cc:231-242, arp.hh:214-216
//   interface's packet provider  src/net/net.cc:266-284
//
// Plain dependent launches on the caller's stream, one tile of kTile items per
// block, no block ever waiting on another one and no atomic deciding a
// position (the only atomics are LDS adds and minima, whose results do not
// depend on their order):
//   eth_rx         eth_rx_count_kernel    class of every frame (-> d_class), the
//                                         tile's per-bucket counts -> workspace
//                  bucket_pass's scan     ONE block (scan_kernel): per bucket an exclusive
//                                         scan over the tiles, the bases -> d_first
//                  eth_rx_scatter_kernel  classes recomputed, offset inside the tile
//                                         (bucket_pass's TileRank), the grouped arrays
//   learn records  compact.h's tile / carry / place kernels over Candidate
//   eth_send       eth_send_count_kernel  per datagram: resolved?, frames, layout
//                                         bytes, descriptors; the tile's totals
//                  eth_send_scan_kernel   ONE block: exclusive scan over the tiles,
//                                         the totals and the capacity cutoff
//                  eth_send_place_kernel  per datagram: status, the unresolved
//                                         list, and per frame its header, position,
//                                         length, source frame and descriptor base
//                  eth_send_emit_kernel   per emitted frame: its descriptors
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <new>
#include <vector>

#include "bucket_pass.h"
#include "compact.h"
#include "host_launch.h"
#include "sccsum.h"
#include "wave_scan.h"
#include "wire.h"

namespace eth {

using bucket_pass::pitch_of;
using host_launch::Chain;
using host_launch::device_ok;
using host_launch::misaligned;
using host_launch::stream_ok;
using host_launch::upload;
using wave_scan::block_inclusive_scan;
using wire::fmix32;
using wire::kIpHdrMin;
using wire::tiles_of;

constexpr int kWave = 64;
constexpr int kBlock = 1024;                 // threads of every tile kernel: one frame / datagram each
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kTile = kBlock;
constexpr uint32_t kMaxProtos = SCCSUM_ETH_MAX_PROTOS;
constexpr uint32_t kMaxBuckets = kMaxProtos + 1;  // the registered protocols + the drop bucket
constexpr uint32_t kEthHdr = 14;             // sizeof(eth_hdr): dst_mac, src_mac, eth_proto
constexpr int kEmitBlock = 256;
constexpr uint32_t kEmitMaxBlocks = 16384;   // the emit grid strides over the frames past this
constexpr uint32_t kMinBits = 4;             // at least 16 slots
constexpr uint64_t kMacMask = 0xFFFFFFFFFFFFull;
constexpr uint64_t kNoCut = ~uint64_t(0);
constexpr int kHostOnly = -1;                // device of a table that has no device copy
// eth_send workspace: [0] frames emitted, [1] datagrams taken (the prefix), then per tile
// {frames, bytes, descriptors, unresolved} (totals, then their exclusive scan)
constexpr uint64_t kWsHead = 4;
constexpr int kQ = 4;

// Home slot of a key in a table of 2^bits slots (bits <= 31).
__host__ __device__ inline uint32_t home_slot(uint32_t ip, uint32_t bits) {
    return fmix32(ip) & ((uint32_t(1) << bits) - 1u);
}

// One slot, 16 bytes: the valid word is apart from the key, so any ip is a key.
struct Slot {
    uint32_t ip;
    uint32_t valid;
    uint64_t mac;
};
static_assert(sizeof(Slot) == 16, "a probe is one 16-byte load");

// What the kernels need of a table (by value in the launch); slots == nullptr maps nothing.
struct Table {
    const Slot* slots;
    uint32_t bits;
};

// Linear probing from the home slot.  The table has at most half of its slots
// taken, so the walk meets an empty one; the trip count is bounded by the
// table's size all the same.
__device__ __forceinline__ bool table_lookup(const Table& T, uint32_t ip, uint64_t* mac) {
    if (!T.slots) return false;
    const uint32_t mask = (uint32_t(1) << T.bits) - 1u;
    uint32_t s = home_slot(ip, T.bits);
    for (uint32_t k = 0; k <= mask; ++k, s = (s + 1u) & mask) {
        const uint4 v = reinterpret_cast<const uint4*>(T.slots)[s];
        if (!v.y) return false;
        if (v.x == ip) {
            *mac = uint64_t(v.z) | (uint64_t(v.w) << 32);
            return true;
        }
    }
    return false;
}

struct Frames {
    const uint8_t* bytes;
    uint64_t bytes_len;
    const uint64_t* off;
    const uint32_t* len;
    uint64_t n;
};

__device__ __forceinline__ bool in_buffer(const Frames& F, uint64_t off, uint32_t len) {
    return off <= F.bytes_len && len <= F.bytes_len - off;
}

// ---------------------------------------------------------------- eth_rx

struct Protos {
    uint16_t v[kMaxProtos];
    uint32_t k;
};

// The class of a frame: k < P.k, or one of the three drop codes.  A frame
// outside the buffer is not read.
__device__ __forceinline__ uint32_t classify(const Frames& F, const Protos& P, uint64_t off, uint32_t len) {
    if (!in_buffer(F, off, len)) return SCCSUM_ETH_RANGE;
    if (len < kEthHdr) return SCCSUM_ETH_SHORT;
    const uint8_t* const h = F.bytes + off;
    const uint32_t proto = (uint32_t(h[12]) << 8) | h[13];
    uint32_t c = SCCSUM_ETH_UNKNOWN;
#pragma unroll
    for (uint32_t k = 0; k < kMaxProtos; ++k) {
        if (k < P.k && P.v[k] == proto) c = k;
    }
    return c;
}

__global__ __launch_bounds__(kBlock) void eth_rx_count_kernel(Frames F, Protos P, uint8_t* __restrict__ d_class,
                                                              uint32_t* __restrict__ ws, uint32_t pitch) {
    __shared__ uint32_t hist[kMaxBuckets];
    bucket_pass::hist_clear(hist);
    __syncthreads();
    const uint64_t i = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    const bool valid = i < F.n;
    const uint32_t c = valid ? classify(F, P, F.off[i], F.len[i]) : SCCSUM_ETH_UNKNOWN;
    const uint32_t b = c < P.k ? c : P.k;
    bucket_pass::hist_add(hist, b, valid);
    if (valid && d_class) d_class[i] = static_cast<uint8_t>(c);
    __syncthreads();
    bucket_pass::hist_store(hist, P.k + 1u, ws, pitch);
}

__global__ __launch_bounds__(kBlock) void eth_rx_scatter_kernel(Frames F, Protos P, const uint32_t* __restrict__ ws,
                                                                uint32_t pitch, const uint32_t* __restrict__ d_first,
                                                                uint32_t* __restrict__ d_order,
                                                                uint64_t* __restrict__ d_l3_off,
                                                                uint32_t* __restrict__ d_l3_len,
                                                                uint64_t* __restrict__ d_src_mac) {
    // base[bucket]: where the tile's frames of the bucket start in the grouped arrays
    __shared__ uint32_t base[kMaxBuckets];
    bucket_pass::TileRank<kWaves, 1, kMaxBuckets> rank;
    rank.clear(P.k + 1u);
    bucket_pass::bucket_base(base, P.k + 1u, d_first, ws, pitch);
    __syncthreads();
    const uint64_t i = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    const bool valid = i < F.n;
    const uint64_t off = valid ? F.off[i] : 0;
    const uint32_t len = valid ? F.len[i] : 0;
    const uint32_t c = valid ? classify(F, P, off, len) : SCCSUM_ETH_UNKNOWN;
    const uint32_t b = c < P.k ? c : P.k;
    rank.mark(0, b, valid);
    __syncthreads();
    rank.scan(P.k + 1u);
    __syncthreads();
    if (!valid) return;
    const uint64_t pos = uint64_t(base[b]) + rank.offset(0, b);
    if (pos >= F.n) return;  // never for consistent inputs
    const bool classified = b < P.k;
    uint64_t mac = 0;
    if (classified) {
        const uint8_t* const h = F.bytes + off + 6;  // eth_hdr::src_mac
#pragma unroll
        for (int k = 0; k < 6; ++k) mac = (mac << 8) | h[k];
    }
    d_order[pos] = static_cast<uint32_t>(i);
    d_l3_off[pos] = classified ? off + kEthHdr : off;
    d_l3_len[pos] = classified ? len - kEthHdr : 0u;
    d_src_mac[pos] = mac;
}

// ---------------------------------------------------------------- learn records

// compact.h's predicate: frame i's record when it is a learn candidate.  The
// caller's status masks, the range and length tests again before the header
// is read, the subnet test of ip.cc:147, then the table.
struct Candidate {
    Frames F;
    const uint8_t* status;
    const uint64_t* mac;
    uint32_t need, reject, host, netmask;
    Table T;

    struct Record {
        uint64_t w[2];  // sccsum_arp_rec as two 64-bit words
    };
    using Out = sccsum_arp_rec;

    __device__ __forceinline__ bool operator()(uint64_t i, Record* rec) const {
        if (i >= F.n) return false;
        if (!wire::status_passes(status[i], need, reject)) return false;
        const uint64_t off = F.off[i];
        const uint32_t len = F.len[i];
        if (!in_buffer(F, off, len) || len < kIpHdrMin) return false;
        const uint32_t src = wire::be32_at(F.bytes + off + 12);  // ip_hdr::src_ip
        if (((src ^ host) & netmask) != 0 || src == host) return false;
        const uint64_t m = mac[i];
        uint64_t known = 0;
        if (table_lookup(T, src, &known) && known == m) return false;
        rec->w[0] = uint64_t(src) | (uint64_t(static_cast<uint32_t>(i)) << 32);
        rec->w[1] = m;
        return true;
    }

    static __device__ __forceinline__ void store(Out* __restrict__ d_rec, uint64_t pos, const Record& rec) {
        uint64_t* const w = reinterpret_cast<uint64_t*>(d_rec + pos);
        w[0] = rec.w[0];
        w[1] = rec.w[1];
    }
};

// ---------------------------------------------------------------- eth_send

struct Send {
    const uint32_t* dst;
    const uint32_t* dfirst;  // nullptr: datagram i is frame i
    uint64_t n;
    const sccsum_gather_desc* desc;
    const uint32_t* first;
    const uint64_t* off;
    const uint32_t* len;
    uint64_t nframes;
    uint32_t host, netmask, gw;
    Table T;
};

// What one datagram asks for: q[] = {frames, layout bytes, descriptors,
// unresolved (0 / 1)}, all 0 for a datagram without a frame, which is not
// looked up; its frames [lo, hi) clamped into the frame arrays.
struct Need {
    uint64_t q[kQ];
    uint64_t mac;
    uint32_t lo, hi, hop;
    bool resolved;
};

__device__ __forceinline__ Need need_of(const Send& S, uint64_t i) {
    Need r{};
    if (i >= S.n) return r;
    uint64_t lo = S.dfirst ? S.dfirst[i] : i;
    uint64_t hi = S.dfirst ? S.dfirst[i + 1] : i + 1;
    if (hi > S.nframes) hi = S.nframes;
    if (lo > hi) lo = hi;
    r.lo = static_cast<uint32_t>(lo);
    r.hi = static_cast<uint32_t>(hi);
    if (lo == hi) return r;
    const uint32_t dst = S.dst[i];
    r.hop = ((dst ^ S.host) & S.netmask) == 0 ? dst : S.gw;  // ip.cc:231-242
    if (!table_lookup(S.T, r.hop, &r.mac)) {
        r.q[3] = 1;
        return r;
    }
    r.resolved = true;
    r.q[0] = hi - lo;
    uint64_t bytes = 0;
    for (uint64_t f = lo; f < hi; ++f) bytes += uint64_t(S.len[f]) + kEthHdr;
    r.q[1] = bytes;
    r.q[2] = uint64_t(S.first[hi] - S.first[lo]) + (hi - lo);
    return r;
}

__global__ __launch_bounds__(kBlock) void eth_send_count_kernel(Send S, uint64_t* __restrict__ ws) {
    __shared__ uint64_t part[kWaves];
    const Need r = need_of(S, uint64_t(blockIdx.x) * kTile + threadIdx.x);
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
        uint64_t total;
        (void)block_inclusive_scan<kWaves>(r.q[q], part, &total);
        if (threadIdx.x == 0) ws[kWsHead + kQ * uint64_t(blockIdx.x) + q] = total;
    }
}

__global__ __launch_bounds__(kBlock) void eth_send_scan_kernel(Send S, uint64_t* __restrict__ ws, uint64_t ntiles,
                                                               uint64_t max_out_bytes,
                                                               uint32_t* __restrict__ d_first_out,
                                                               uint64_t* __restrict__ d_total) {
    __shared__ uint64_t part[kWaves];
    __shared__ unsigned long long cut_tile;  // the first tile past which the cap is exceeded
    __shared__ unsigned int cut_slot;        // the first datagram of that tile that does not fit
    __shared__ uint64_t at_cut[kQ];
    if (threadIdx.x == 0) {
        cut_tile = kNoCut;
        cut_slot = kTile;
    }
    __syncthreads();
    uint64_t carry[kQ] = {0, 0, 0, 0};  // carried over the chunks of 1024 tiles
    for (uint64_t base = 0; base < ntiles; base += kBlock) {
        const uint64_t t = base + threadIdx.x;
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            const uint64_t v = t < ntiles ? ws[kWsHead + kQ * t + q] : 0;
            uint64_t sum;
            const uint64_t incl = carry[q] + block_inclusive_scan<kWaves>(v, part, &sum);
            if (t < ntiles) {
                ws[kWsHead + kQ * t + q] = incl - v;
                if (q == 1 && incl > max_out_bytes) atomicMin(&cut_tile, static_cast<unsigned long long>(t));
            }
            carry[q] += sum;
        }
    }
    __syncthreads();
    const uint64_t tc = cut_tile;
    uint64_t prefix = S.n, frames = carry[0], descs = carry[2], unres = carry[3];
    if (tc != kNoCut) {
        // the cap falls inside tile tc: its datagrams once more, on top of its base
        const Need r = need_of(S, tc * kTile + threadIdx.x);
        uint64_t excl[kQ];
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
            uint64_t total;
            excl[q] = ws[kWsHead + kQ * tc + q] + block_inclusive_scan<kWaves>(r.q[q], part, &total) - r.q[q];
        }
        if (excl[1] + r.q[1] > max_out_bytes) atomicMin(&cut_slot, threadIdx.x);
        __syncthreads();
        const uint32_t k = cut_slot;  // < kTile: the tile's total does not fit
        if (threadIdx.x == k) {
#pragma unroll
            for (int q = 0; q < kQ; ++q) at_cut[q] = excl[q];
        }
        __syncthreads();
        prefix = tc * kTile + k;
        frames = at_cut[0];
        descs = at_cut[2];
        unres = at_cut[3];
    }
    if (threadIdx.x == 0) {
        ws[0] = frames;
        ws[1] = prefix;
        d_total[0] = carry[0];
        d_total[1] = carry[1];
        d_total[2] = prefix;
        d_total[3] = unres;
        d_total[4] = frames;
        d_total[5] = descs;
        if (frames <= S.nframes) d_first_out[frames] = static_cast<uint32_t>(descs);  // the closing entry
    }
}

struct SendOut {
    uint8_t* eth;
    sccsum_gather_desc* desc;
    uint32_t* first;
    uint64_t* off;
    uint32_t* len;
    uint32_t* frame_src;
    uint8_t* status;
    sccsum_eth_unresolved* unresolved;
};

__global__ __launch_bounds__(kBlock) void eth_send_place_kernel(Send S, const uint64_t* __restrict__ ws,
                                                                uint64_t hw_address, uint32_t eth_proto, SendOut O) {
    __shared__ uint64_t part[kWaves];
    const uint64_t prefix = ws[1];
    const uint64_t i = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    const Need r = need_of(S, i);
    uint64_t at[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
        uint64_t total;
        at[q] = ws[kWsHead + kQ * uint64_t(blockIdx.x) + q] + block_inclusive_scan<kWaves>(r.q[q], part, &total) -
                r.q[q];
    }
    if (i >= S.n) return;
    const bool taken = i < prefix;
    O.status[i] = static_cast<uint8_t>(!taken ? 0u : r.resolved ? SCCSUM_ST_OK : r.q[3] ? SCCSUM_ST_NOARP : 0u);
    if (!taken) return;
    if (r.q[3]) {
        *reinterpret_cast<uint64_t*>(O.unresolved + at[3]) = uint64_t(static_cast<uint32_t>(i)) | (uint64_t(r.hop) << 32);
    }
    if (!r.resolved) return;
    uint8_t hdr[kEthHdr];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        hdr[k] = static_cast<uint8_t>(r.mac >> (40 - 8 * k));
        hdr[6 + k] = static_cast<uint8_t>(hw_address >> (40 - 8 * k));
    }
    hdr[12] = static_cast<uint8_t>(eth_proto >> 8);
    hdr[13] = static_cast<uint8_t>(eth_proto);
    uint64_t fo = at[0], bo = at[1], de = at[2];
    for (uint32_t f = r.lo; f < r.hi && fo < S.nframes; ++f, ++fo) {  // fo < nframes always, for consistent inputs
        const uint32_t len = S.len[f];
        uint8_t* const e = O.eth + fo * kEthHdr;
#pragma unroll
        for (uint32_t k = 0; k < kEthHdr; ++k) e[k] = hdr[k];
        O.frame_src[fo] = f;
        O.off[fo] = bo;
        O.len[fo] = len + kEthHdr;  // fits: the frame's bytes are inside max_out_bytes <= 2^32 - 1
        O.first[fo] = static_cast<uint32_t>(de);
        bo += uint64_t(len) + kEthHdr;
        de += uint64_t(S.first[f + 1] - S.first[f]) + 1u;
    }
}

static_assert(sizeof(sccsum_gather_desc) == 16 && offsetof(sccsum_gather_desc, dst_off) == 8 &&
                  offsetof(sccsum_gather_desc, len) == 12,
              "the emit kernel moves a descriptor as two 64-bit words");
static_assert(sizeof(sccsum_eth_unresolved) == 8 && sizeof(sccsum_arp_rec) == 16 && sizeof(sccsum_arp_entry) == 16,
              "records are stored as 64-bit words");

// One emitted frame per thread: the Ethernet descriptor, then the frame's own
// descriptors moved behind it.
__global__ __launch_bounds__(kEmitBlock) void eth_send_emit_kernel(Send S, const uint64_t* __restrict__ ws, SendOut O) {
    const uint64_t emitted = ws[0];
    for (uint64_t g = uint64_t(blockIdx.x) * kEmitBlock + threadIdx.x; g < emitted;
         g += uint64_t(gridDim.x) * kEmitBlock) {
        const uint32_t f = O.frame_src[g];
        const uint32_t at = static_cast<uint32_t>(O.off[g]);
        const uint32_t shift = at + kEthHdr - static_cast<uint32_t>(S.off[f]);
        const uint32_t lo = S.first[f], hi = S.first[f + 1];
        uint64_t* out = reinterpret_cast<uint64_t*>(O.desc + O.first[g]);
        out[0] = reinterpret_cast<uint64_t>(O.eth + g * kEthHdr);
        out[1] = uint64_t(at) | (uint64_t(kEthHdr) << 32);
        const uint64_t* in = reinterpret_cast<const uint64_t*>(S.desc + lo);
        for (uint32_t j = lo; j < hi; ++j) {
            out += 2;
            const uint64_t w = in[1];
            out[0] = in[0];
            out[1] = uint64_t(static_cast<uint32_t>(w) + shift) | (w & 0xFFFFFFFF00000000ull);
            in += 2;
        }
    }
}

// ---------------------------------------------------------------- host side

uint32_t bits_for(uint32_t n) {
    uint32_t bits = kMinBits;
    while ((uint64_t(1) << bits) < 2 * uint64_t(n)) ++bits;
    return bits;
}

bool entries_ok(const sccsum_arp_entry* entries, uint32_t n) {
    if (n > SCCSUM_ARP_MAX_ENTRIES || (n != 0 && !entries)) return false;
    for (uint32_t i = 0; i < n; ++i) {
        if (entries[i].mac & ~kMacMask) return false;
    }
    return true;
}

// The entries in order into an empty table: a key met again takes the later MAC.
std::vector<Slot> build_slots(const sccsum_arp_entry* entries, uint32_t n, uint32_t bits) {
    std::vector<Slot> slots(size_t(1) << bits, Slot{0, 0, 0});
    const uint32_t mask = (uint32_t(1) << bits) - 1u;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t s = home_slot(entries[i].ip, bits);
        while (slots[s].valid && slots[s].ip != entries[i].ip) s = (s + 1u) & mask;
        slots[s] = Slot{entries[i].ip, 1u, entries[i].mac};
    }
    return slots;
}

}  // namespace eth

struct sccsum_arp_table {
    int device = eth::kHostOnly;
    uint32_t bits = eth::kMinBits;
    std::vector<eth::Slot> slots;     // the host copy sccsum_arp_table_lookup walks
    eth::Slot* d_slots = nullptr;     // the device copy (none for a host-only table)
};

namespace eth {

int new_table(const sccsum_arp_entry* entries, uint32_t n, sccsum_arp_table** out) {
    auto* t = new (std::nothrow) sccsum_arp_table;
    if (!t) return static_cast<int>(hipErrorOutOfMemory);
    t->bits = bits_for(n);
    t->slots = build_slots(entries, n, t->bits);
    *out = t;
    return SCCSUM_OK;
}

// The device view of a table for a launch; nullptr maps nothing.
Table view(const sccsum_arp_table* t) { return t ? Table{t->d_slots, t->bits} : Table{nullptr, kMinBits}; }

}  // namespace eth

extern "C" {

int sccsum_eth_tile_packets(void) { return static_cast<int>(eth::kTile); }

uint32_t sccsum_arp_table_slot(uint32_t ip, uint32_t bits) {
    return bits > 31 ? UINT32_MAX : eth::home_slot(ip, bits);
}

uint32_t sccsum_arp_table_bits(const sccsum_arp_table* t) { return t ? t->bits : 0; }

int sccsum_arp_table_create_host(const sccsum_arp_entry* entries, uint32_t n, sccsum_arp_table** out) {
    if (!out) return SCCSUM_EINVAL;
    *out = nullptr;
    if (!eth::entries_ok(entries, n)) return SCCSUM_EINVAL;
    return eth::new_table(entries, n, out);
}

int sccsum_arp_table_create(int device, const sccsum_arp_entry* entries, uint32_t n, sccsum_arp_table** out) {
    using namespace eth;
    if (!out) return SCCSUM_EINVAL;
    *out = nullptr;
    if (!entries_ok(entries, n)) return SCCSUM_EINVAL;
    int rc = device_ok(device);
    if (rc != SCCSUM_OK) return rc;
    sccsum_arp_table* t = nullptr;
    rc = new_table(entries, n, &t);
    if (rc != SCCSUM_OK) return rc;
    void* d[1];
    rc = upload(device, {{t->slots.data(), t->slots.size() * sizeof(Slot)}}, d);
    if (rc != SCCSUM_OK) {
        delete t;
        return rc;
    }
    t->d_slots = static_cast<Slot*>(d[0]);
    t->device = device;
    *out = t;
    return SCCSUM_OK;
}

int sccsum_arp_table_destroy(sccsum_arp_table* t) {
    if (!t) return SCCSUM_OK;
    const hipError_t e = host_launch::free_all({t->d_slots});
    delete t;
    return static_cast<int>(e);
}

int sccsum_arp_table_lookup(const sccsum_arp_table* t, uint32_t ip, uint64_t* mac) {
    if (!t || !mac) return 0;
    const uint32_t mask = (uint32_t(1) << t->bits) - 1u;
    for (uint32_t s = eth::home_slot(ip, t->bits); t->slots[s].valid; s = (s + 1u) & mask) {
        if (t->slots[s].ip == ip) {
            *mac = t->slots[s].mac;
            return 1;
        }
    }
    return 0;
}

uint64_t sccsum_eth_rx_workspace(uint64_t n) {
    const uint64_t pitch = eth::pitch_of(eth::tiles_of(n, eth::kTile));
    return eth::kMaxBuckets * pitch * 4u + 16u;  // the per-tile counts [9][pitch]
}

int sccsum_eth_rx(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len, uint64_t n,
                  const uint16_t* protos, uint32_t nprotos, uint8_t* d_class, uint32_t* d_first, uint32_t* d_order,
                  uint64_t* d_l3_off, uint32_t* d_l3_len, uint64_t* d_src_mac, void* d_workspace, void* stream) {
    using namespace eth;
    if (!protos || nprotos < 1 || nprotos > kMaxProtos || n > 0xFFFFFFFFull) return SCCSUM_EINVAL;
    Protos P{};
    P.k = nprotos;
    for (uint32_t k = 0; k < nprotos; ++k) {
        for (uint32_t j = 0; j < k; ++j) {
            if (protos[j] == protos[k]) return SCCSUM_EINVAL;
        }
        P.v[k] = protos[k];
    }
    if (!d_first || !d_workspace || misaligned(d_first, 4) || misaligned(d_workspace, 16)) return SCCSUM_EINVAL;
    if (n != 0) {
        if ((!d_bytes && bytes_len != 0) || !d_off || !d_len || !d_order || !d_l3_off || !d_l3_len || !d_src_mac) {
            return SCCSUM_EINVAL;
        }
        if (misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_order, 4) || misaligned(d_l3_off, 8) ||
            misaligned(d_l3_len, 4) || misaligned(d_src_mac, 8)) {
            return SCCSUM_EINVAL;
        }
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, -1);
    if (rc != SCCSUM_OK) return rc;

    const Frames F{static_cast<const uint8_t*>(d_bytes), bytes_len, d_off, d_len, n};
    const uint32_t ntiles = static_cast<uint32_t>(tiles_of(n, kTile));
    const uint32_t pitch = pitch_of(ntiles);
    uint32_t* const ws = static_cast<uint32_t*>(d_workspace);
    Chain c{st};
    if (ntiles) c.launch(eth_rx_count_kernel, dim3(ntiles), dim3(kBlock), 0, F, P, d_class, ws, pitch);
    // at most nine buckets: always the one-block scan, which leaves no totals behind the rows
    static_assert(kMaxBuckets <= bucket_pass::kScanOneBlockMax, "sccsum_eth_rx_workspace has no room for totals");
    if (c.ok()) c.e = bucket_pass::scan_buckets<kBlock, kMaxBuckets>(st, ws, ntiles, pitch, nprotos + 1u, d_first, nullptr);
    if (!ntiles) return c.rc();
    c.launch(eth_rx_scatter_kernel, dim3(ntiles), dim3(kBlock), 0, F, P, ws, pitch, d_first, d_order, d_l3_off, d_l3_len,
             d_src_mac);
    return c.rc();
}

uint64_t sccsum_arp_learn_workspace(uint64_t n) {
    return (eth::tiles_of(n, eth::kTile) * 4u + 15u + 16u) & ~uint64_t(15);
}

int sccsum_arp_learn_records(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                             const uint8_t* d_status, uint32_t need, uint32_t reject, const uint64_t* d_src_mac,
                             uint64_t n, uint32_t host, uint32_t netmask, const sccsum_arp_table* table,
                             sccsum_arp_rec* d_rec, uint32_t* d_count, void* d_workspace, void* stream) {
    using namespace eth;
    if (n > 0x7FFFFFFFull || (need | reject) > 0xFFu) return SCCSUM_EINVAL;
    if (!d_count || !d_workspace || misaligned(d_count, 4) || misaligned(d_workspace, 16)) return SCCSUM_EINVAL;
    if (n != 0) {
        if ((!d_bytes && bytes_len != 0) || !d_off || !d_len || !d_status || !d_src_mac || !d_rec) return SCCSUM_EINVAL;
        if (misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_src_mac, 8) || misaligned(d_rec, 8)) {
            return SCCSUM_EINVAL;
        }
    }
    if (table && table->device == kHostOnly) return SCCSUM_ENODEV;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, table ? table->device : -1);
    if (rc != SCCSUM_OK) return rc;

    const Candidate C{Frames{static_cast<const uint8_t*>(d_bytes), bytes_len, d_off, d_len, n}, d_status, d_src_mac,
                      need, reject, host, netmask, view(table)};
    return static_cast<int>(
        compact::run<kBlock>(st, C, tiles_of(n, kTile), static_cast<uint32_t*>(d_workspace), d_count, d_rec));
}

uint64_t sccsum_eth_send_workspace(uint64_t n) {
    return ((eth::kWsHead + eth::kQ * eth::tiles_of(n, eth::kTile)) * 8u + 15u) & ~uint64_t(15);
}

int sccsum_eth_send(const sccsum_eth_opts* opts, const sccsum_arp_table* table, const uint32_t* d_dst,
                    const uint32_t* d_dgram_first, uint64_t n, const sccsum_gather_desc* d_desc,
                    const uint32_t* d_first, const uint64_t* d_off, const uint32_t* d_len, uint64_t nframes,
                    uint64_t max_out_bytes, uint8_t* d_eth, sccsum_gather_desc* d_desc_out, uint32_t* d_first_out,
                    uint64_t* d_off_out, uint32_t* d_len_out, uint32_t* d_frame_src, uint8_t* d_status,
                    sccsum_eth_unresolved* d_unresolved, uint64_t* d_total, void* d_workspace, void* stream) {
    using namespace eth;
    if (!opts || (opts->hw_address & ~kMacMask) || !table) return SCCSUM_EINVAL;
    if (n > 0xFFFFFFFFull || nframes > 0x7FFFFFFFull || max_out_bytes > 0xFFFFFFFFull) return SCCSUM_EINVAL;
    if (!d_dgram_first && nframes != n) return SCCSUM_EINVAL;
    if (!d_total || !d_first_out || !d_workspace) return SCCSUM_EINVAL;
    if (misaligned(d_total, 8) || misaligned(d_first_out, 4) || misaligned(d_workspace, 16) ||
        misaligned(d_dgram_first, 4)) {
        return SCCSUM_EINVAL;
    }
    if (n != 0) {
        if (!d_dst || !d_status || !d_unresolved) return SCCSUM_EINVAL;
        if (misaligned(d_dst, 4) || misaligned(d_unresolved, 8)) return SCCSUM_EINVAL;
    }
    if (nframes != 0) {
        // d_desc may be NULL when no frame has a descriptor, as in the *_desc calls
        if (!d_first || !d_off || !d_len || !d_eth || !d_desc_out || !d_off_out || !d_len_out ||
            !d_frame_src) {
            return SCCSUM_EINVAL;
        }
        if (misaligned(d_desc, 8) || misaligned(d_first, 4) || misaligned(d_off, 8) || misaligned(d_len, 4) ||
            misaligned(d_desc_out, 8) || misaligned(d_off_out, 8) || misaligned(d_len_out, 4) ||
            misaligned(d_frame_src, 4)) {
            return SCCSUM_EINVAL;
        }
    }
    if (table->device == kHostOnly) return SCCSUM_ENODEV;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, table->device);
    if (rc != SCCSUM_OK) return rc;

    const Send S{d_dst, d_dgram_first, n, d_desc, d_first, d_off, d_len, nframes, opts->host, opts->netmask,
                 opts->gw, view(table)};
    const SendOut O{d_eth, d_desc_out, d_first_out, d_off_out, d_len_out, d_frame_src, d_status, d_unresolved};
    const uint64_t ntiles = tiles_of(n, kTile);
    uint64_t* const ws = static_cast<uint64_t*>(d_workspace);
    const dim3 tiles(static_cast<unsigned>(ntiles)), block(kBlock);
    Chain c{st};
    if (ntiles) c.launch(eth_send_count_kernel, tiles, block, 0, S, ws);
    c.launch(eth_send_scan_kernel, dim3(1), block, 0, S, ws, ntiles, max_out_bytes, d_first_out, d_total);
    if (!ntiles) return c.rc();
    c.launch(eth_send_place_kernel, tiles, block, 0, S, ws, opts->hw_address, uint32_t(opts->eth_proto), O);
    if (!nframes) return c.rc();
    const uint64_t blocks = std::min<uint64_t>((nframes + kEmitBlock - 1) / kEmitBlock, kEmitMaxBlocks);
    c.launch(eth_send_emit_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kEmitBlock), 0, S, ws, O);
    return c.rc();
}

}  // extern "C"
