// tcp.hip — the TCP layer above the IPv4 path on the GPU: on rx the stateless
// part of tcp::received for a batch (the header found and its data_offset
// checked, the twenty fixed bytes read, the connid looked up in the connection
// table, then the listening ports, then the RST of respond_with_reset), ending
// in segments grouped per connection with their headers parsed; on tx
// tcb::output_one's header written into the payload's headroom (sccsum.h, "TCP
// layer").
//
// What it restates from the reference (paths relative to the reference tree):
//   tcp_hdr::read / write          include/seastar/net/tcp.hh:246-282
//   tcp::received                  tcp.hh:865-942
//   tcp::respond_with_reset        tcp.hh:981-1023
//   tcb::output_one, the header    tcp.hh:1620-1698
//   ipv4::handle_received_packet   src/net/ip.cc:159-162, 222-227
//
// Plain dependent launches on the caller's stream, one tile of kTile items per
// block, no block ever waiting on another one and no atomic deciding a
// position (the only atomics are LDS adds, whose sums do not depend on their
// order):
//   tcp_rx   decode_kernel    every frame decoded once: its class (-> d_class), its
//                             32-byte record and its two addresses (-> the workspace),
//                             its sort key and call position (-> the workspace), the
//                             tile's counts of the key's lowest digit
//            per 8-bit digit  scan_rows_kernel, sort_scatter_kernel (a stable LSD
//                             radix pass over (key, position) pairs), and
//                             sort_count_kernel for the next digit
//            gather_kernel    the sorted pairs read in order: d_order, d_seg, d_src
//                             (coalesced stores, the records gathered), the bucket
//                             bases -> d_first, the tile's count of run heads
//            run_carry_kernel one block: the tiles' counts become prefixes; d_total,
//                             the closing entry of d_run_first
//            run_place_kernel d_run_conn, d_run_first
//            reset_kernel     the answers of bucket 2 -> d_rst, d_rst_dst (tcp_reset.h)
//   The key is the connection index for bucket 0 and nconns + 0 / 1 / 2 for
//   buckets 1 to 3, so ONE sort yields the grouped order and the bucket bases:
//   one pass up to 253 connections, two up to 65 533, three beyond.
//   tcp_send                  send_kernel, one segment per thread
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <new>
#include <vector>

#include "bucket_pass.h"
#include "host_launch.h"
#include "sccsum.h"
#include "tcp_reset.h"
#include "wave_scan.h"
#include "wire.h"

namespace tcp {

using bucket_pass::kDigits;
using bucket_pass::scan_rows_kernel;
using host_launch::Chain;
using host_launch::device_ok;
using host_launch::misaligned;
using host_launch::stream_ok;
using host_launch::upload;
using host_launch::Workspace;
using wave_scan::block_inclusive_scan;
using wire::be16_at;
using wire::be32_at;
using wire::pseudo_seed;
using wire::tiles_of;

constexpr int kWave = 64;
constexpr int kBlock = 1024;                 // threads of every tile kernel: one segment each
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kTile = kBlock;           // sccsum_eth_tile_packets()
constexpr uint32_t kPorts = 65536;
constexpr uint32_t kTcpHdr = 20;             // tcp_hdr::len
constexpr uint32_t kProtoTcp = 6;
constexpr uint32_t kMaxL4 = 65515;           // sccsum_ipv4_send's limit
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kRst = 4u;
constexpr int kFlatBlock = 256;
constexpr int kHostOnly = -1;                // device of a table that has no device copy
constexpr uint32_t kMaxConns = SCCSUM_TCP_MAX_CONNS;

static_assert(sizeof(sccsum_tcp_seg) == 32 && sizeof(sccsum_tcp_out) == 24 && sizeof(sccsum_tcp_conn) == 12, "layout");

// ---------------------------------------------------------------- the connection table

// The home slot of a connid (wire.h: tcp_listen.hip's table takes the same one).
__host__ __device__ inline uint32_t hash_of(uint32_t local_ip, uint32_t foreign_ip, uint32_t ports) {
    return wire::connid_hash(local_ip, foreign_ip, ports);
}

// Linear probing from the home slot: the connection index, or kNone at the
// first empty slot.  At most half of the slots are taken, so one is met.
__host__ __device__ inline uint32_t probe(const uint4* __restrict__ slots, uint32_t mask, uint32_t local_ip,
                                          uint32_t foreign_ip, uint32_t ports) {
    uint32_t s = hash_of(local_ip, foreign_ip, ports) & mask;
    for (uint32_t k = 0; k <= mask; ++k) {
        const uint4 e = slots[s];  // one 16-byte load
        if (e.w == 0) return kNone;
        if (e.x == local_ip && e.y == foreign_ip && e.z == ports) return e.w - 1u;
        s = (s + 1u) & mask;
    }
    return kNone;
}

// ---------------------------------------------------------------- rx: what one frame is

// The sort key's bucket part: connection c is key c, buckets 1..3 follow the connections.
__device__ __forceinline__ uint32_t bucket_of_key(uint32_t key, uint32_t nconns) {
    return key < nconns ? 0u : key - nconns + 1u;
}

struct Decode {
    const uint8_t* bytes;
    uint64_t bytes_len;
    const uint64_t* off;
    const uint32_t* len;
    uint64_t nbatch;
    const uint8_t* status;
    const uint32_t* index;
    uint64_t n;
    uint32_t need, reject, host;
    const uint4* slots;
    uint32_t mask, nconns;
    const uint8_t* listening;
};

// What the decode leaves of frame j in the workspace: the record as d_seg
// takes it, with the batch frame index where `conn` will stand (conn is the
// key's), and the two addresses.
struct Item {
    uint32_t cls, key;
    uint64_t pay_off;
    uint32_t pay_len, seq, ack, index;
    uint32_t window, sport, dport, flags, hdr_len;
    uint32_t src, dst;
};

// Frame j of the call is batch frame index[j] (j itself without an index):
// sccsum_udp_rx's SKIP rules with protocol 6, then tcp.hh:866-874, 884-898.
__device__ __forceinline__ Item decode(const Decode& D, uint64_t j) {
    Item it{};
    it.cls = SCCSUM_TCP_SKIP;
    it.key = D.nconns + 2u;
    it.index = D.index ? D.index[j] : static_cast<uint32_t>(j);
    const uint64_t i = it.index;
    if (i >= D.nbatch) return it;
    const uint64_t o = D.off[i];
    const uint32_t l = D.len[i];
    const uint32_t st = D.status[i];
    it.pay_off = o;
    if (!wire::status_passes(st, D.need, D.reject)) return it;
    wire::Ipv4View ip;
    if (!wire::ipv4_view(D.bytes, D.bytes_len, o, l, &ip)) return it;
    if ((ip.frag & 0x3FFFu) != 0) return it;              // MF or a fragment offset
    const uint32_t dst = ip.dst();
    if (D.host != 0 && dst != D.host) return it;
    if (ip.proto() != kProtoTcp) return it;
    const uint32_t ihl4 = ip.hdr_len;
    const uint32_t E = ip.ip_len - ihl4;                  // the trim to the IP total length
    it.cls = SCCSUM_TCP_SHORT;
    if (E < kTcpHdr) return it;                           // get_header(0, tcp_hdr::len) is null
    const uint8_t* const t = ip.h + ihl4;
    const uint32_t H = 4u * (uint32_t(t[12]) >> 4);
    if (H < kTcpHdr) return it;
    const uint32_t src = ip.src();
    const uint32_t sport = be16_at(t), dport = be16_at(t + 2);
    const uint32_t flags = t[13];
    const uint32_t c = probe(D.slots, D.mask, dst, src, (dport << 16) | sport);
    if (c != kNone) {
        if (H > E) return it;                             // the options are not in the segment: dropped
        it.cls = SCCSUM_TCP_CONN;
        it.key = c;
    } else if (D.listening[dport]) {
        if (H > E) return it;
        it.cls = SCCSUM_TCP_LISTEN;
        it.key = D.nconns;
    } else if (flags & kRst) {
        it.cls = SCCSUM_TCP_NOCONN;
    } else {
        it.cls = SCCSUM_TCP_RESET;
        it.key = D.nconns + 1u;
    }
    it.pay_off = o + ihl4 + H;
    it.pay_len = E > H ? E - H : 0u;
    it.seq = be32_at(t + 4);
    it.ack = be32_at(t + 8);
    it.window = be16_at(t + 14);
    it.sport = sport;
    it.dport = dport;
    it.flags = flags;
    it.hdr_len = H;
    it.src = src;
    it.dst = dst;
    return it;
}

// sccsum_tcp_seg as two 16-byte words: {pay_off, pay_len, seq}, {ack, conn,
// window | sport << 16, dport | flags << 16 | hdr_len << 24}.
__device__ __forceinline__ void store_item(uint4* __restrict__ rec, uint64_t j, const Item& it) {
    rec[2 * j] = make_uint4(static_cast<uint32_t>(it.pay_off), static_cast<uint32_t>(it.pay_off >> 32), it.pay_len,
                            it.seq);
    rec[2 * j + 1] = make_uint4(it.ack, it.index, it.window | (it.sport << 16),
                                it.dport | (it.flags << 16) | (it.hdr_len << 24));
}

__global__ __launch_bounds__(kBlock) void decode_kernel(Decode D, uint8_t* __restrict__ d_class,
                                                        uint4* __restrict__ rec, uint2* __restrict__ addr,
                                                        uint2* __restrict__ kv, uint32_t* __restrict__ counts,
                                                        uint32_t pitch) {
    __shared__ uint32_t hist[kDigits];
    bucket_pass::hist_clear(hist);
    __syncthreads();
    const uint64_t j = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    const bool valid = j < D.n;
    uint32_t key = 0;
    if (valid) {
        const Item it = decode(D, j);
        key = it.key;
        store_item(rec, j, it);
        addr[j] = make_uint2(it.src, it.dst);
        kv[j] = make_uint2(key, static_cast<uint32_t>(j));
        if (d_class) d_class[j] = static_cast<uint8_t>(it.cls);
    }
    bucket_pass::hist_add(hist, key & 0xFFu, valid);
    __syncthreads();
    bucket_pass::hist_store(hist, kDigits, counts, pitch);
}

// ---------------------------------------------------------------- rx: one radix pass

__global__ __launch_bounds__(kBlock) void sort_count_kernel(const uint2* __restrict__ kv, uint64_t n, int shift,
                                                            uint32_t* __restrict__ counts, uint32_t pitch) {
    __shared__ uint32_t hist[kDigits];
    bucket_pass::hist_clear(hist);
    __syncthreads();
    const uint64_t p = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    const bool valid = p < n;
    const uint32_t key = valid ? kv[p].x : 0u;
    bucket_pass::hist_add(hist, (key >> shift) & 0xFFu, valid);
    __syncthreads();
    bucket_pass::hist_store(hist, kDigits, counts, pitch);
}

// Stable: a pair's position is its digit's base, the pairs of the digit in the
// tiles before (counts), and its offset among them inside the tile.
__global__ __launch_bounds__(kBlock) void sort_scatter_kernel(const uint2* __restrict__ kv, uint64_t n, int shift,
                                                              const uint32_t* __restrict__ counts, uint32_t pitch,
                                                              const uint32_t* __restrict__ totals,
                                                              uint2* __restrict__ kv_out) {
    __shared__ uint32_t base[kDigits];
    __shared__ uint32_t part[kWaves];
    bucket_pass::TileRank<kWaves, 1, kDigits> rank;
    bucket_pass::digit_base<kWaves>(base, totals, counts, pitch, part);
    rank.clear(kDigits);
    __syncthreads();
    const uint64_t p = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    const bool valid = p < n;
    const uint2 e = valid ? kv[p] : make_uint2(0, 0);
    const uint32_t d = (e.x >> shift) & 0xFFu;
    rank.mark(0, d, valid);
    __syncthreads();
    rank.scan(kDigits);
    __syncthreads();
    if (!valid) return;
    const uint64_t pos = uint64_t(base[d]) + rank.offset(0, d);
    if (pos < n) kv_out[pos] = e;  // always true: the counts are this pass's own
}

// ---------------------------------------------------------------- rx: the grouped arrays, the runs, the resets

struct RxOut {
    uint32_t* first;      // [5]
    uint32_t* order;
    uint2* seg;           // sccsum_tcp_seg as four 8-byte words: d_seg is 8-byte aligned
    uint32_t* src;
    uint32_t* run_conn;
    uint32_t* run_first;
    uint32_t* rst;        // 20 bytes = five words per answer
    uint32_t* rst_dst;
    uint64_t* total;      // [4]
};

// Sorted position p starts a run of bucket 0: its key is a connection and differs from the key before.
__device__ __forceinline__ bool run_head(const uint2* __restrict__ kv, uint64_t p, uint32_t key, uint32_t nconns) {
    return key < nconns && (p == 0 || kv[p - 1].x != key);
}

__global__ __launch_bounds__(kBlock) void gather_kernel(const uint2* __restrict__ kv, uint64_t n, uint32_t nconns,
                                                        const uint4* __restrict__ rec, const uint2* __restrict__ addr,
                                                        RxOut O, uint32_t* __restrict__ tcount) {
    __shared__ uint32_t part[kWaves];
    const uint64_t p = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    uint32_t head = 0;
    if (p < n) {
        const uint2 e = kv[p];
        const uint32_t b = bucket_of_key(e.x, nconns);
        uint4 lo = rec[2 * uint64_t(e.y)], hi = rec[2 * uint64_t(e.y) + 1];
        O.order[p] = hi.y;
        hi.y = b == 0 ? e.x : kNone;
        O.seg[4 * p] = make_uint2(lo.x, lo.y);
        O.seg[4 * p + 1] = make_uint2(lo.z, lo.w);
        O.seg[4 * p + 2] = make_uint2(hi.x, hi.y);
        O.seg[4 * p + 3] = make_uint2(hi.z, hi.w);
        O.src[p] = addr[e.y].x;
        head = run_head(kv, p, e.x, nconns) ? 1u : 0u;
        // every base is written once: by the first position of a bucket for the buckets
        // up to its own that are still open, by the last position for the rest
        const uint32_t before = p == 0 ? 0u : bucket_of_key(kv[p - 1].x, nconns) + 1u;
        for (uint32_t k = before; k <= b; ++k) O.first[k] = static_cast<uint32_t>(p);
        if (p + 1 == n) {
            for (uint32_t k = b + 1u; k <= 4u; ++k) O.first[k] = static_cast<uint32_t>(n);
        }
    }
    uint32_t total;
    (void)block_inclusive_scan<kWaves>(head, part, &total);
    if (threadIdx.x == 0) tcount[blockIdx.x] = total;
}

// ONE block: the per-tile run counts become inclusive prefixes in place; R and
// the resets -> d_total, the closing entry of d_run_first.
__global__ __launch_bounds__(kBlock) void run_carry_kernel(uint32_t* __restrict__ tcount, uint32_t ntiles, RxOut O) {
    __shared__ uint32_t part[kWaves];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < ntiles; base += kBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < ntiles ? tcount[t] : 0u;
        uint32_t total;
        const uint32_t incl = carry + block_inclusive_scan<kWaves>(v, part, &total);
        if (t < ntiles) tcount[t] = incl;
        carry += total;
    }
    if (threadIdx.x == 0) {
        if (ntiles == 0) {
            for (int k = 0; k < 5; ++k) O.first[k] = 0;
        }
        const uint32_t f1 = ntiles ? O.first[1] : 0u;
        O.run_first[carry] = f1;
        O.total[0] = carry;
        O.total[1] = ntiles ? O.first[3] - O.first[2] : 0u;
        O.total[2] = 0;
        O.total[3] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void run_place_kernel(const uint2* __restrict__ kv, uint64_t n, uint32_t nconns,
                                                           const uint32_t* __restrict__ tcount, RxOut O) {
    __shared__ uint32_t part[kWaves];
    const uint64_t p = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    const uint32_t key = p < n ? kv[p].x : kNone;
    const bool head = p < n && run_head(kv, p, key, nconns);
    uint32_t total;
    const uint32_t incl = block_inclusive_scan<kWaves>(head ? 1u : 0u, part, &total);
    if (!head) return;
    const uint64_t r = uint64_t(blockIdx.x ? tcount[blockIdx.x - 1] : 0u) + incl - 1u;
    O.run_conn[r] = key;
    O.run_first[r] = static_cast<uint32_t>(p);
}

// respond_with_reset (tcp.hh:981-1023) for the r-th segment of bucket 2.
__global__ __launch_bounds__(kFlatBlock) void reset_kernel(const uint2* __restrict__ kv,
                                                           const uint2* __restrict__ addr, uint32_t flags, RxOut O) {
    const uint32_t lo = O.first[2], hi = O.first[3];
    const uint64_t p = uint64_t(lo) + uint64_t(blockIdx.x) * kFlatBlock + threadIdx.x;
    if (p >= hi) return;
    const uint64_t r = p - lo;
    const uint2 a = O.seg[4 * p + 1], b = O.seg[4 * p + 2], c = O.seg[4 * p + 3];
    const uint2 ad = addr[kv[p].y];                        // x = src (the foreign address), y = dst (ours)
    tcp_reset::answer(a.y, b.x, c.x >> 16, c.y & 0xFFFFu, (c.y >> 16) & 0xFFu, ad.x, ad.y, flags, O.rst + 5 * r,
                      O.rst_dst + r);
}

// ---------------------------------------------------------------- tx: tcp_send

struct Send {
    uint8_t* bytes;
    uint64_t bytes_len;
    const uint64_t* off;
    const uint32_t* len;
    const uint32_t* out;  // sccsum_tcp_out as six words
    uint64_t n;
    uint32_t src_host, flags;
};

struct SendOut {
    uint64_t* l4_off;
    uint32_t* l4_len;
    uint32_t* sum_len;
    uint32_t* seed;
    uint16_t* tso_seg;
    uint8_t* proto;  // optional
    uint8_t* needs_csum;
    uint8_t* status;
};

// tcp.hh:1620-1698 for segment i: the twenty fixed bytes in front of the
// options the caller wrote, and what the checksum pass and ipv4::send take.
__global__ __launch_bounds__(kFlatBlock) void send_kernel(Send S, SendOut O) {
    const uint64_t i = uint64_t(blockIdx.x) * kFlatBlock + threadIdx.x;
    if (i >= S.n) return;
    const uint64_t off = S.off[i];
    const uint32_t len = S.len[i];
    const uint32_t* const q = S.out + 6 * i;
    const uint32_t dst = q[0], seq = q[1], ack = q[2], w3 = q[3], w4 = q[4], mss = q[5];
    const uint32_t sport = w3 & 0xFFFFu, dport = w3 >> 16, window = w4 & 0xFFFFu;
    const uint32_t flags = (w4 >> 16) & 0xFFu, hdr_len = w4 >> 24;
    uint32_t st = 0;
    if (off < hdr_len || off > S.bytes_len || len > S.bytes_len - off) st |= SCCSUM_ST_RANGE;
    if (hdr_len < kTcpHdr || hdr_len > 60u || (hdr_len & 3u) || uint64_t(len) + hdr_len > kMaxL4) st |= SCCSUM_ST_MALFORMED;
    if ((S.flags & SCCSUM_TCP_TSO) && mss == 0) st |= SCCSUM_ST_MALFORMED;
    if (O.proto) O.proto[i] = static_cast<uint8_t>(kProtoTcp);
    if (st) {
        O.status[i] = static_cast<uint8_t>(st);
        O.l4_off[i] = ~uint64_t(0);
        O.l4_len[i] = 0;
        O.sum_len[i] = 0;
        O.seed[i] = 0;
        O.tso_seg[i] = 0;
        O.needs_csum[i] = 0;
        return;
    }
    const uint32_t l4_len = len + hdr_len;
    uint8_t* const h = S.bytes + (off - hdr_len);
    h[0] = static_cast<uint8_t>(sport >> 8);
    h[1] = static_cast<uint8_t>(sport);
    h[2] = static_cast<uint8_t>(dport >> 8);
    h[3] = static_cast<uint8_t>(dport);
    h[4] = static_cast<uint8_t>(seq >> 24);
    h[5] = static_cast<uint8_t>(seq >> 16);
    h[6] = static_cast<uint8_t>(seq >> 8);
    h[7] = static_cast<uint8_t>(seq);
    h[8] = static_cast<uint8_t>(ack >> 24);
    h[9] = static_cast<uint8_t>(ack >> 16);
    h[10] = static_cast<uint8_t>(ack >> 8);
    h[11] = static_cast<uint8_t>(ack);
    h[12] = static_cast<uint8_t>((hdr_len / 4u) << 4);
    h[13] = static_cast<uint8_t>(flags);
    h[14] = static_cast<uint8_t>(window >> 8);
    h[15] = static_cast<uint8_t>(window);
    h[16] = 0;
    h[17] = 0;
    h[18] = 0;
    h[19] = 0;
    const bool offload = (S.flags & SCCSUM_TCP_CSUM_OFFLOAD) != 0;           // tcp.hh:1662
    const bool tso = offload && (S.flags & SCCSUM_TCP_TSO) && len > mss;     // tcp.hh:1674
    const uint32_t seed = pseudo_seed(S.src_host, dst, kProtoTcp, tso ? 0u : l4_len);
    O.status[i] = static_cast<uint8_t>(SCCSUM_ST_OK);
    O.l4_off[i] = off - hdr_len;
    O.l4_len[i] = l4_len;
    // offload: the empty span's result is the folded pseudo-header sum itself, ~csum.get() (tcp.hh:1689)
    O.sum_len[i] = offload ? 0u : l4_len;
    O.seed[i] = offload ? (0xFFFFu ^ seed) : seed;
    O.tso_seg[i] = tso ? static_cast<uint16_t>(mss) : uint16_t(0);
    O.needs_csum[i] = offload ? 1 : 0;
}

// ---------------------------------------------------------------- host side

uint32_t slot_bits(uint32_t nconns) {
    uint32_t bits = 4;
    while ((uint64_t(1) << bits) < 2ull * nconns) ++bits;
    return bits;
}

// The 8-bit digits of the largest key, nconns + 2.
int passes_of(uint32_t nconns) {
    const uint32_t top = nconns + 2u;
    return top < (1u << 8) ? 1 : top < (1u << 16) ? 2 : 3;
}

}  // namespace tcp

struct sccsum_tcp_conns {
    int device = tcp::kHostOnly;
    uint32_t nconns = 0, bits = 4;
    std::vector<uint4> slots;       // the host copy sccsum_tcp_conns_lookup reads
    std::vector<uint8_t> listening; // port -> 1 / 0
    uint4* d_slots = nullptr;       // the device copies (none for a host-only table)
    uint8_t* d_listening = nullptr;
};

namespace tcp {

// SCCSUM_EINVAL rules first, then the object with its host copies; a connid or a port given twice is refused.
int new_conns(const sccsum_tcp_conn* conns, uint32_t nconns, const uint16_t* listen, uint32_t nlisten,
              sccsum_tcp_conns** out) {
    if (nconns > kMaxConns || (nconns != 0 && !conns) || nlisten > kPorts || (nlisten != 0 && !listen)) {
        return SCCSUM_EINVAL;
    }
    auto* t = new (std::nothrow) sccsum_tcp_conns;
    if (!t) return static_cast<int>(hipErrorOutOfMemory);
    t->nconns = nconns;
    t->bits = slot_bits(nconns);
    const uint32_t mask = (1u << t->bits) - 1u;
    t->slots.assign(size_t(1) << t->bits, make_uint4(0, 0, 0, 0));
    t->listening.assign(kPorts, 0);
    for (uint32_t c = 0; c < nconns; ++c) {
        const uint32_t ports = (uint32_t(conns[c].local_port) << 16) | conns[c].foreign_port;
        uint32_t s = hash_of(conns[c].local_ip, conns[c].foreign_ip, ports) & mask;
        while (t->slots[s].w != 0) {
            const uint4 e = t->slots[s];
            if (e.x == conns[c].local_ip && e.y == conns[c].foreign_ip && e.z == ports) {
                delete t;
                return SCCSUM_EINVAL;
            }
            s = (s + 1u) & mask;
        }
        t->slots[s] = make_uint4(conns[c].local_ip, conns[c].foreign_ip, ports, c + 1u);
    }
    for (uint32_t k = 0; k < nlisten; ++k) {
        if (t->listening[listen[k]]) {
            delete t;
            return SCCSUM_EINVAL;
        }
        t->listening[listen[k]] = 1;
    }
    *out = t;
    return SCCSUM_OK;
}

// The workspace: 16-byte things first.
struct Layout {
    uint64_t rec, addr, kv0, kv1, counts, totals, tcount, bytes;
    uint32_t ntiles, pitch;
};

Layout layout_of(uint64_t n) {
    Layout L{};
    L.ntiles = static_cast<uint32_t>(tiles_of(n, kTile));
    L.pitch = bucket_pass::pitch_of(L.ntiles);
    host_launch::Carver c;
    L.rec = c.take(32 * n);
    L.addr = c.take(8 * n);
    L.kv0 = c.take(8 * n);
    L.kv1 = c.take(8 * n);
    L.counts = c.take(uint64_t(kDigits) * L.pitch * 4u, 16);
    L.totals = c.take(kDigits * 4u);
    L.tcount = c.take((uint64_t(L.ntiles) + 4u) * 4u);
    L.bytes = c.end();
    return L;
}

}  // namespace tcp

extern "C" {

int sccsum_tcp_conns_create_host(const sccsum_tcp_conn* conns, uint32_t nconns, const uint16_t* listen,
                                 uint32_t nlisten, sccsum_tcp_conns** out) {
    if (!out) return SCCSUM_EINVAL;
    *out = nullptr;
    return tcp::new_conns(conns, nconns, listen, nlisten, out);
}

int sccsum_tcp_conns_create(int device, const sccsum_tcp_conn* conns, uint32_t nconns, const uint16_t* listen,
                            uint32_t nlisten, sccsum_tcp_conns** out) {
    using namespace tcp;
    if (!out) return SCCSUM_EINVAL;
    *out = nullptr;
    sccsum_tcp_conns* t = nullptr;
    int rc = new_conns(conns, nconns, listen, nlisten, &t);   // duplicates show only while the table is built
    if (rc != SCCSUM_OK) return rc;
    void* d[2];
    rc = device_ok(device);
    if (rc == SCCSUM_OK) {
        rc = upload(device, {{t->slots.data(), t->slots.size() * sizeof(uint4)}, {t->listening.data(), kPorts}}, d);
    }
    if (rc != SCCSUM_OK) {
        delete t;
        return rc;
    }
    t->d_slots = static_cast<uint4*>(d[0]);
    t->d_listening = static_cast<uint8_t*>(d[1]);
    t->device = device;
    *out = t;
    return SCCSUM_OK;
}

int sccsum_tcp_conns_destroy(sccsum_tcp_conns* t) {
    if (!t) return SCCSUM_OK;
    const hipError_t e = host_launch::free_all({t->d_slots, t->d_listening});
    delete t;
    return static_cast<int>(e);
}

int64_t sccsum_tcp_conns_lookup(const sccsum_tcp_conns* t, uint32_t local_ip, uint32_t foreign_ip, uint16_t local_port,
                                uint16_t foreign_port) {
    if (!t) return -1;
    const uint32_t c = tcp::probe(t->slots.data(), (1u << t->bits) - 1u, local_ip, foreign_ip,
                                  (uint32_t(local_port) << 16) | foreign_port);
    return c == tcp::kNone ? -1 : static_cast<int64_t>(c);
}

int sccsum_tcp_conns_listening(const sccsum_tcp_conns* t, uint16_t port) { return t && t->listening[port] ? 1 : 0; }

uint32_t sccsum_tcp_conns_slot(uint32_t local_ip, uint32_t foreign_ip, uint16_t local_port, uint16_t foreign_port,
                               uint32_t bits) {
    const uint32_t h = tcp::hash_of(local_ip, foreign_ip, (uint32_t(local_port) << 16) | foreign_port);
    return bits >= 32 ? h : h & ((1u << bits) - 1u);
}

uint32_t sccsum_tcp_conns_bits(const sccsum_tcp_conns* t) { return t ? t->bits : 0; }
uint32_t sccsum_tcp_conns_count(const sccsum_tcp_conns* t) { return t ? t->nconns : 0; }

uint64_t sccsum_tcp_rx_workspace(uint64_t n, uint32_t nconns) {
    (void)nconns;  // the sort's buffers do not depend on the number of passes
    return tcp::layout_of(n).bytes;
}

int sccsum_tcp_rx(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                  uint64_t nbatch, const uint8_t* d_status, uint32_t need, uint32_t reject, uint32_t host_address,
                  const sccsum_tcp_conns* conns, const uint32_t* d_index, uint64_t n, uint32_t flags, uint8_t* d_class,
                  uint32_t* d_first, uint32_t* d_order, sccsum_tcp_seg* d_seg, uint32_t* d_src, uint32_t* d_run_conn,
                  uint32_t* d_run_first, void* d_rst, uint32_t* d_rst_dst, uint64_t* d_total, void* d_workspace,
                  void* stream) {
    using namespace tcp;
    if (!conns || (need | reject) > 0xFFu || n > 0xFFFFFFFFull || nbatch > 0xFFFFFFFFull) return SCCSUM_EINVAL;
    if (flags & ~uint32_t(SCCSUM_TCP_CSUM_OFFLOAD)) return SCCSUM_EINVAL;
    if (!d_index && n > nbatch) return SCCSUM_EINVAL;
    if (!d_first || !d_run_first || !d_total || !d_workspace) return SCCSUM_EINVAL;
    if (misaligned(d_first, 4) || misaligned(d_run_first, 4) || misaligned(d_total, 8) || misaligned(d_workspace, 16)) {
        return SCCSUM_EINVAL;
    }
    if (n != 0) {
        if (!d_order || !d_seg || !d_src || !d_run_conn || !d_rst || !d_rst_dst) return SCCSUM_EINVAL;
        if (nbatch != 0 && ((!d_bytes && bytes_len != 0) || !d_off || !d_len || !d_status)) return SCCSUM_EINVAL;
        if (misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_index, 4) || misaligned(d_order, 4) ||
            misaligned(d_seg, 8) || misaligned(d_src, 4) || misaligned(d_run_conn, 4) || misaligned(d_rst, 4) ||
            misaligned(d_rst_dst, 4)) {
            return SCCSUM_EINVAL;
        }
    }
    if (conns->device == kHostOnly) return SCCSUM_ENODEV;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, conns->device);
    if (rc != SCCSUM_OK) return rc;

    const Layout L = layout_of(n);
    const Workspace ws(d_workspace);
    uint4* const rec = ws.at<uint4>(L.rec);
    uint2* const addr = ws.at<uint2>(L.addr);
    uint2* kv = ws.at<uint2>(L.kv0);
    uint2* kv_other = ws.at<uint2>(L.kv1);
    uint32_t* const counts = ws.u32(L.counts);
    uint32_t* const totals = ws.u32(L.totals);
    uint32_t* const tcount = ws.u32(L.tcount);
    const RxOut O{d_first, d_order, reinterpret_cast<uint2*>(d_seg), d_src, d_run_conn, d_run_first,
                  static_cast<uint32_t*>(d_rst), d_rst_dst, d_total};
    const uint32_t nconns = conns->nconns;
    const dim3 tiles(L.ntiles), block(kBlock);
    Chain c{st};
    if (L.ntiles) {
        const Decode D{static_cast<const uint8_t*>(d_bytes), bytes_len, d_off, d_len, nbatch, d_status, d_index, n,
                       need, reject, host_address, conns->d_slots, (1u << conns->bits) - 1u, nconns,
                       conns->d_listening};
        c.launch(decode_kernel, tiles, block, 0, D, d_class, rec, addr, kv, counts, L.pitch);
        const int passes = passes_of(nconns);
        for (int p = 0; p < passes; ++p) {
            if (p != 0) c.launch(sort_count_kernel, tiles, block, 0, kv, n, 8 * p, counts, L.pitch);
            c.launch(scan_rows_kernel<>, dim3(kDigits), dim3(kWave), 0, counts, L.ntiles, L.pitch, totals);
            c.launch(sort_scatter_kernel, tiles, block, 0, kv, n, 8 * p, counts, L.pitch, totals, kv_other);
            uint2* const t = kv;
            kv = kv_other;
            kv_other = t;
        }
        c.launch(gather_kernel, tiles, block, 0, kv, n, nconns, rec, addr, O, tcount);
    }
    c.launch(run_carry_kernel, dim3(1), block, 0, tcount, L.ntiles, O);
    if (!L.ntiles) return c.rc();
    c.launch(run_place_kernel, tiles, block, 0, kv, n, nconns, tcount, O);
    const uint64_t blocks = (n + kFlatBlock - 1) / kFlatBlock;
    c.launch(reset_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kFlatBlock), 0, kv, addr, flags, O);
    return c.rc();
}

int sccsum_tcp_send(const sccsum_tcp_opts* opts, void* d_bytes, uint64_t bytes_len, const uint64_t* d_off,
                    const uint32_t* d_len, const sccsum_tcp_out* d_out, uint64_t n, uint64_t* d_l4_off,
                    uint32_t* d_l4_len, uint32_t* d_sum_len, uint32_t* d_seed, uint16_t* d_tso_seg, uint8_t* d_proto,
                    uint8_t* d_needs_csum, uint8_t* d_status, void* stream) {
    using namespace tcp;
    if (!opts || opts->mtu < 68 || opts->mtu > 65535) return SCCSUM_EINVAL;
    if (opts->flags & ~uint32_t(SCCSUM_TCP_CSUM_OFFLOAD | SCCSUM_TCP_TSO)) return SCCSUM_EINVAL;
    if (n > 0xFFFFFFFFull) return SCCSUM_EINVAL;
    if (n != 0) {
        if ((!d_bytes && bytes_len != 0) || !d_off || !d_len || !d_out || !d_l4_off || !d_l4_len || !d_sum_len ||
            !d_seed || !d_tso_seg || !d_needs_csum || !d_status) {
            return SCCSUM_EINVAL;
        }
        if (misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_out, 4) || misaligned(d_l4_off, 8) ||
            misaligned(d_l4_len, 4) || misaligned(d_sum_len, 4) || misaligned(d_seed, 4) || misaligned(d_tso_seg, 2)) {
            return SCCSUM_EINVAL;
        }
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, -1);
    if (rc != SCCSUM_OK || n == 0) return rc;
    const Send S{static_cast<uint8_t*>(d_bytes), bytes_len, d_off, d_len, reinterpret_cast<const uint32_t*>(d_out), n,
                 opts->src_host, opts->flags};
    const SendOut O{d_l4_off, d_l4_len, d_sum_len, d_seed, d_tso_seg, d_proto, d_needs_csum, d_status};
    const uint64_t blocks = (n + kFlatBlock - 1) / kFlatBlock;
    Chain c{st};
    c.launch(send_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kFlatBlock), 0, S, O);
    return c.rc();
}

}  // extern "C"
