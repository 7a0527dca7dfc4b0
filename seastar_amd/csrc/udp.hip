// udp.hip — the UDP layer above the IPv4 path on the GPU: on rx the last steps
// of ipv4::handle_received_packet and ipv4_udp::received for a batch (is it for
// us, is it UDP, the trim to the IP length, the two headers dropped, the channel
// by destination port), for atomic frames and for reassembled datagrams; on tx
// ipv4_udp::send's header written into the payload's headroom (sccsum.h, "UDP
// layer").
//
// What it restates from the reference (paths relative to the reference tree):
//   ipv4::handle_received_packet   src/net/ip.cc:159-162, 222-227
//   native_datagram, received      src/net/udp.cc:45-53, 164-173
//   ipv4_udp::send                 src/net/udp.cc:175-197
//   ipv4::needs_frag               src/net/ip.cc:100-111
//
// Plain dependent launches on the caller's stream, one tile of kTile items per
// block, no block ever waiting on another one and no atomic deciding a
// position (the only atomics are LDS adds, whose sums do not depend on their
// order):
//   udp_rx / udp_rx_reasm  count_kernel<Decode>    every item decoded: its class (->
//                                                  d_class), what the grouped arrays
//                                                  say of it (-> a 16-byte stash in
//                                                  the workspace), the tile's
//                                                  per-bucket counts
//                          scan kernels            per bucket an exclusive scan over
//                                                  the tiles, the bases -> d_first
//                          scatter_kernel<Decode>  the stash read back (no header is
//                                                  read twice), rank inside the tile
//                                                  from wave match masks, the grouped
//                                                  arrays
//   Decode is FramesDecode (a frame of an IPv4 bucket, read where it lies) or
//   ReasmDecode (a reassembled datagram: its head record and the first eight
//   bytes of its fragment list).
//   udp_send               send_kernel             one datagram per thread
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <new>
#include <vector>

#include "bucket_pass.h"
#include "host_launch.h"
#include "sccsum.h"
#include "wire.h"

namespace udp {

using bucket_pass::pitch_of;
using host_launch::Chain;
using host_launch::device_ok;
using host_launch::misaligned;
using host_launch::stream_ok;
using host_launch::upload;
using wire::be16_at;
using wire::kIpHdrMin;
using wire::pseudo_seed;
using wire::status_passes;
using wire::tiles_of;

constexpr int kWave = 64;
constexpr int kBlock = 1024;                 // threads of every tile kernel: one frame / datagram each
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kTile = kBlock;           // sccsum_eth_tile_packets()
constexpr uint32_t kMaxChannels = SCCSUM_UDP_MAX_CHANNELS;
constexpr uint32_t kMaxBuckets = kMaxChannels + 1;  // the channels + the drop bucket
constexpr uint32_t kTotals = 256;            // the bucket totals of the many-bucket scan, behind the rows
constexpr uint32_t kPorts = 65536;
constexpr uint32_t kUnbound = 0xFF;
constexpr uint32_t kUdpHdr = 8;              // sizeof(udp_hdr): src_port, dst_port, len, cksum
constexpr uint32_t kProtoUdp = 17;
constexpr uint32_t kMaxPayload = 65507;      // ipv4_send's 65 515 less the header
constexpr int kSendBlock = 256;
constexpr int kHostOnly = -1;                // device of a table that has no device copy

static_assert(kMaxBuckets <= 256 && kMaxChannels <= SCCSUM_UDP_SKIP, "a bucket and a class are 8 bits");

// ---------------------------------------------------------------- rx: what one item is

// One frame / datagram of a call: its class, the index it is listed under, and
// what the grouped arrays say of it (0, 0, 0 for a dropped one); `add` is where
// the payload starts behind the item's own offset (0 for a dropped one).
struct Item {
    uint32_t cls;
    uint32_t index;
    uint32_t add;
    uint32_t pay_len, src, sport;
};

// What the count kernel leaves of an item for the scatter kernel, so that the
// frame's header is read once: 16 bytes, stored and loaded as one.
//   x = src, y = sport | pay_len << 16 (both 16 bits: an IP length is),
//   z = class | add << 8, w = index
__device__ __forceinline__ uint4 stash_of(const Item& it) {
    return make_uint4(it.src, it.sport | (it.pay_len << 16), it.cls | (it.add << 8), it.index);
}

// The channel of an 8-byte UDP header: one byte load from the port table.
__device__ __forceinline__ uint32_t channel_of(const uint8_t* __restrict__ table, uint32_t dport) {
    const uint32_t k = table[dport];
    return k == kUnbound ? uint32_t(SCCSUM_UDP_NOPORT) : k;
}

// Frame j of the call is batch frame index[j] (j itself without an index):
// the caller's status masks, the range and header-trust tests before anything
// behind them is read, then ip.cc:159-162 (destination), 164 (fragments are
// reassembly's), 222 (protocol), 225-226 (trim to the IP length, drop the IP
// header) and udp.cc:45-53, 168-169.
struct FramesDecode {
    const uint8_t* bytes;
    uint64_t bytes_len;
    const uint64_t* off;
    const uint32_t* len;
    uint64_t nbatch;
    const uint8_t* status;
    const uint32_t* index;
    uint64_t n;
    uint32_t need, reject, host;
    const uint8_t* table;

    __device__ __forceinline__ Item operator()(uint64_t j) const {
        Item it{SCCSUM_UDP_SKIP, static_cast<uint32_t>(j), 0, 0, 0, 0};
        if (index) it.index = index[j];
        const uint64_t i = it.index;
        if (i >= nbatch) return it;
        const uint64_t o = off[i];
        const uint32_t l = len[i];
        if (!status_passes(status[i], need, reject)) return it;
        wire::Ipv4View ip;
        if (!wire::ipv4_view(bytes, bytes_len, o, l, &ip)) return it;
        if ((ip.frag & 0x3FFFu) != 0) return it;              // MF or a fragment offset
        if (host != 0 && ip.dst() != host) return it;
        if (ip.proto() != kProtoUdp) return it;
        const uint32_t l4_len = ip.ip_len - ip.hdr_len;       // the trim to the IP total length
        if (l4_len < kUdpHdr) {
            it.cls = SCCSUM_UDP_SHORT;
            return it;
        }
        const uint8_t* const u = ip.h + ip.hdr_len;
        it.cls = channel_of(table, be16_at(u + 2));
        if (it.cls >= kMaxChannels) return it;
        it.add = ip.hdr_len + kUdpHdr;
        it.pay_len = l4_len - kUdpHdr;                         // udp_hdr::len is not consulted
        it.src = ip.src();
        it.sport = be16_at(u);
        return it;
    }

    // Where batch frame i lies: what d_pay_off counts from (0 for an index out of range).
    __device__ __forceinline__ uint64_t base(uint32_t i) const { return i < nbatch ? off[i] : 0; }
};

// Datagram d of sccsum_ipv4_reasm's output: addresses and protocol from its
// head record, the UDP header's eight bytes through its fragment list.
struct ReasmDecode {
    const sccsum_gather_desc* desc;
    const uint32_t* first;
    const uint64_t* off;
    const uint32_t* len;
    const uint32_t* head;
    uint64_t n;
    const sccsum_frag_rec* rec;
    uint64_t nrec;
    const uint8_t* l4_status;
    uint32_t need, reject, host;
    const uint8_t* table;

    __device__ __forceinline__ Item operator()(uint64_t d) const {
        Item it{SCCSUM_UDP_SKIP, static_cast<uint32_t>(d), 0, 0, 0, 0};
        if (l4_status && !status_passes(l4_status[d], need, reject)) return it;
        const uint64_t hi = head[d];
        if (hi >= nrec) return it;
        const uint64_t* const w = reinterpret_cast<const uint64_t*>(rec + hi);
        const uint64_t addr = w[1];                            // src | dst << 32
        const uint32_t proto = static_cast<uint32_t>((w[2] >> 16) & 0xFFu);
        const uint32_t dst = static_cast<uint32_t>(addr >> 32);
        if (host != 0 && dst != host) return it;
        if (proto != kProtoUdp) return it;
        const uint32_t E = len[d];
        if (E < kUdpHdr) {
            it.cls = SCCSUM_UDP_SHORT;
            return it;
        }
        // layout bytes [off, off + 8): at most eight descriptors hold them, none read past the list's end
        const uint32_t lo = first[d], end = first[d + 1];
        const uint32_t at = static_cast<uint32_t>(off[d]);    // dst_off is the low 32 bits of a layout position
        uint32_t hdr[kUdpHdr / 2] = {0, 0, 0, 0};
        uint32_t got = 0;
        for (uint32_t k = 0; k < kUdpHdr && lo + k < end && lo <= end; ++k) {
            const uint64_t* const q = reinterpret_cast<const uint64_t*>(desc + lo + k);
            const uint8_t* const src = reinterpret_cast<const uint8_t*>(q[0]);
            const uint32_t rel = static_cast<uint32_t>(q[1]) - at;
            const uint32_t dl = static_cast<uint32_t>(q[1] >> 32);
#pragma unroll
            for (uint32_t b = 0; b < kUdpHdr; ++b) {
                if (b >= rel && b - rel < dl) {
                    const uint32_t v = src[b - rel];
                    hdr[b / 2] = (b & 1u) ? (hdr[b / 2] & 0xFF00u) | v : (hdr[b / 2] & 0x00FFu) | (v << 8);
                    got |= 1u << b;
                }
            }
        }
        if (got != 0xFFu) return it;                           // the list does not tile the header: not trusted
        it.cls = channel_of(table, hdr[1]);
        if (it.cls >= kMaxChannels) return it;
        it.pay_len = E - kUdpHdr;
        it.src = static_cast<uint32_t>(addr);
        it.sport = hdr[0];
        return it;
    }

    __device__ __forceinline__ uint64_t base(uint32_t) const { return 0; }  // no d_pay_off: the payload is the list's
};

// ---------------------------------------------------------------- rx: count / scan / scatter

template <typename Decode>
__global__ __launch_bounds__(kBlock) void count_kernel(Decode dec, uint32_t channels, uint8_t* __restrict__ d_class,
                                                       uint4* __restrict__ stash, uint32_t* __restrict__ ws,
                                                       uint32_t pitch) {
    __shared__ uint32_t hist[kMaxBuckets];
    bucket_pass::hist_clear(hist);
    __syncthreads();
    const uint64_t j = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    const bool valid = j < dec.n;
    Item it{SCCSUM_UDP_SKIP, 0, 0, 0, 0, 0};
    if (valid) {
        it = dec(j);
        stash[j] = stash_of(it);
    }
    const uint32_t c = it.cls;
    const uint32_t b = c < channels ? c : channels;
    bucket_pass::hist_add(hist, b, valid);
    if (valid && d_class) d_class[j] = static_cast<uint8_t>(c);
    __syncthreads();
    bucket_pass::hist_store(hist, channels + 1u, ws, pitch);
}

struct RxOut {
    uint32_t* order;
    uint64_t* pay_off;  // nullptr for reassembled datagrams: the payload is the list's bytes from +8
    uint32_t* pay_len;
    uint32_t* src;
    uint16_t* sport;
};

template <typename Decode>
__global__ __launch_bounds__(kBlock) void scatter_kernel(Decode dec, uint32_t channels, const uint4* __restrict__ stash,
                                                         const uint32_t* __restrict__ ws, uint32_t pitch,
                                                         const uint32_t* __restrict__ d_first, RxOut O) {
    // base[bucket]: where the tile's items of the bucket start in the grouped arrays
    __shared__ uint32_t base[kMaxBuckets];
    bucket_pass::TileRank<kWaves, 1, kMaxBuckets> rank;
    rank.clear(channels + 1u);
    bucket_pass::bucket_base(base, channels + 1u, d_first, ws, pitch);
    __syncthreads();
    const uint64_t j = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    const bool valid = j < dec.n;
    uint4 it = make_uint4(0, 0, SCCSUM_UDP_SKIP, 0);
    if (valid) it = stash[j];
    const uint32_t cls = it.z & 0xFFu;
    const uint32_t b = cls < channels ? cls : channels;
    rank.mark(0, b, valid);
    __syncthreads();
    rank.scan(channels + 1u);
    __syncthreads();
    if (!valid) return;
    const uint64_t pos = uint64_t(base[b]) + rank.offset(0, b);
    if (pos >= dec.n) return;  // never for consistent inputs
    O.order[pos] = it.w;
    if (O.pay_off) O.pay_off[pos] = dec.base(it.w) + (it.z >> 8);
    O.pay_len[pos] = it.y >> 16;
    O.src[pos] = it.x;
    O.sport[pos] = static_cast<uint16_t>(it.y);
}

// ---------------------------------------------------------------- tx: udp_send

struct Send {
    uint8_t* bytes;
    uint64_t bytes_len;
    const uint64_t* off;
    const uint32_t* len;
    const uint32_t* dst;
    const uint16_t* dport;
    const uint16_t* sport;
    uint64_t n;
    uint32_t src_host, mtu, flags;
};

struct SendOut {
    uint64_t* l4_off;
    uint32_t* l4_len;
    uint32_t* sum_len;
    uint32_t* seed;
    uint8_t* proto;  // optional
    uint8_t* needs_csum;
    uint8_t* status;
};

// udp.cc:175-197 for datagram i: the header into the eight bytes in front of
// the payload, and what the checksum pass and ipv4::send take of it.
__global__ __launch_bounds__(kSendBlock) void send_kernel(Send S, SendOut O) {
    const uint64_t i = uint64_t(blockIdx.x) * kSendBlock + threadIdx.x;
    if (i >= S.n) return;
    const uint64_t off = S.off[i];
    const uint32_t len = S.len[i];
    uint32_t st = 0;
    if (off < kUdpHdr || off > S.bytes_len || len > S.bytes_len - off) st |= SCCSUM_ST_RANGE;
    if (len > kMaxPayload) st |= SCCSUM_ST_MALFORMED;
    if (O.proto) O.proto[i] = static_cast<uint8_t>(kProtoUdp);
    if (st) {
        O.status[i] = static_cast<uint8_t>(st);
        O.l4_off[i] = ~uint64_t(0);
        O.l4_len[i] = 0;
        O.sum_len[i] = 0;
        O.seed[i] = 0;
        O.needs_csum[i] = 0;
        return;
    }
    const uint32_t l4_len = len + kUdpHdr;
    const uint32_t sport = S.sport[i], dport = S.dport[i];
    uint8_t* const h = S.bytes + (off - kUdpHdr);
    h[0] = static_cast<uint8_t>(sport >> 8);
    h[1] = static_cast<uint8_t>(sport);
    h[2] = static_cast<uint8_t>(dport >> 8);
    h[3] = static_cast<uint8_t>(dport);
    h[4] = static_cast<uint8_t>(l4_len >> 8);
    h[5] = static_cast<uint8_t>(l4_len);
    h[6] = 0;
    h[7] = 0;
    const bool needs_frag = l4_len + kIpHdrMin > S.mtu && !(S.flags & SCCSUM_UDP_UFO);  // ip.cc:100-111
    const bool offload = (S.flags & SCCSUM_UDP_CSUM_OFFLOAD) && !needs_frag;            // udp.cc:188
    const uint32_t seed = pseudo_seed(S.src_host, S.dst[i], kProtoUdp, l4_len);
    O.status[i] = static_cast<uint8_t>(SCCSUM_ST_OK);
    O.l4_off[i] = off - kUdpHdr;
    O.l4_len[i] = l4_len;
    // offload: the empty span's result is the folded pseudo-header sum itself, ~csum.get() (udp.cc:189)
    O.sum_len[i] = offload ? 0u : l4_len;
    O.seed[i] = offload ? (0xFFFFu ^ seed) : seed;
    O.needs_csum[i] = offload ? 1 : 0;
}

// ---------------------------------------------------------------- host side

}  // namespace udp

struct sccsum_udp_ports {
    int device = udp::kHostOnly;
    uint32_t channels = 0;
    std::vector<uint8_t> table;   // port -> channel, 0xFF unbound: the host copy sccsum_udp_ports_lookup reads
    uint8_t* d_table = nullptr;   // the device copy (none for a host-only table)
};

namespace udp {

bool ports_ok(const uint16_t* ports, uint32_t channels) {
    if (channels > kMaxChannels || (channels != 0 && !ports)) return false;
    bool seen[kPorts] = {};
    for (uint32_t k = 0; k < channels; ++k) {
        if (seen[ports[k]]) return false;
        seen[ports[k]] = true;
    }
    return true;
}

int new_ports(const uint16_t* ports, uint32_t channels, sccsum_udp_ports** out) {
    auto* t = new (std::nothrow) sccsum_udp_ports;
    if (!t) return static_cast<int>(hipErrorOutOfMemory);
    t->channels = channels;
    t->table.assign(kPorts, static_cast<uint8_t>(kUnbound));
    for (uint32_t k = 0; k < channels; ++k) t->table[ports[k]] = static_cast<uint8_t>(k);
    *out = t;
    return SCCSUM_OK;
}

uint64_t rx_workspace(uint64_t n) {
    const uint64_t pitch = pitch_of(tiles_of(n, kTile));
    // one 16-byte stash per item, the per-tile counts [253][pitch], then the bucket totals
    return 16u * n + (kMaxBuckets * pitch + kTotals) * 4u;
}

// count, scan, scatter over the n items `dec` decodes.
template <typename Decode>
int run_rx(const Decode& dec, uint32_t channels, uint8_t* d_class, uint32_t* d_first, const RxOut& O, void* d_workspace,
           hipStream_t st) {
    const uint32_t ntiles = static_cast<uint32_t>(tiles_of(dec.n, kTile));
    const uint32_t pitch = pitch_of(ntiles);
    const uint32_t buckets = channels + 1u;
    uint4* const stash = static_cast<uint4*>(d_workspace);
    uint32_t* const ws = reinterpret_cast<uint32_t*>(stash + dec.n);
    Chain c{st};
    if (ntiles) c.launch(count_kernel<Decode>, dim3(ntiles), dim3(kBlock), 0, dec, channels, d_class, stash, ws, pitch);
    if (c.ok()) {
        c.e = bucket_pass::scan_buckets<kBlock, kMaxBuckets>(st, ws, ntiles, pitch, buckets, d_first,
                                                             ws + uint64_t(kMaxBuckets) * pitch);
    }
    if (!ntiles) return c.rc();
    c.launch(scatter_kernel<Decode>, dim3(ntiles), dim3(kBlock), 0, dec, channels, stash, ws, pitch, d_first, O);
    return c.rc();
}

}  // namespace udp

extern "C" {

int sccsum_udp_ports_create_host(const uint16_t* ports, uint32_t channels, sccsum_udp_ports** out) {
    if (!out) return SCCSUM_EINVAL;
    *out = nullptr;
    if (!udp::ports_ok(ports, channels)) return SCCSUM_EINVAL;
    return udp::new_ports(ports, channels, out);
}

int sccsum_udp_ports_create(int device, const uint16_t* ports, uint32_t channels, sccsum_udp_ports** out) {
    using namespace udp;
    if (!out) return SCCSUM_EINVAL;
    *out = nullptr;
    if (!ports_ok(ports, channels)) return SCCSUM_EINVAL;
    int rc = device_ok(device);
    if (rc != SCCSUM_OK) return rc;
    sccsum_udp_ports* t = nullptr;
    rc = new_ports(ports, channels, &t);
    if (rc != SCCSUM_OK) return rc;
    void* d[1];
    rc = upload(device, {{t->table.data(), kPorts}}, d);
    if (rc != SCCSUM_OK) {
        delete t;
        return rc;
    }
    t->d_table = static_cast<uint8_t*>(d[0]);
    t->device = device;
    *out = t;
    return SCCSUM_OK;
}

int sccsum_udp_ports_destroy(sccsum_udp_ports* t) {
    if (!t) return SCCSUM_OK;
    const hipError_t e = host_launch::free_all({t->d_table});
    delete t;
    return static_cast<int>(e);
}

int sccsum_udp_ports_lookup(const sccsum_udp_ports* t, uint16_t port) {
    if (!t) return -1;
    const uint32_t k = t->table[port];
    return k == udp::kUnbound ? -1 : static_cast<int>(k);
}

uint32_t sccsum_udp_ports_channels(const sccsum_udp_ports* t) { return t ? t->channels : 0; }

uint64_t sccsum_udp_rx_workspace(uint64_t n) { return udp::rx_workspace(n); }
uint64_t sccsum_udp_rx_reasm_workspace(uint64_t m) { return udp::rx_workspace(m); }

int sccsum_udp_rx(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                  uint64_t nbatch, const uint8_t* d_status, uint32_t need, uint32_t reject, uint32_t host_address,
                  const sccsum_udp_ports* ports, const uint32_t* d_index, uint64_t n, uint8_t* d_class,
                  uint32_t* d_first, uint32_t* d_order, uint64_t* d_pay_off, uint32_t* d_pay_len, uint32_t* d_src,
                  uint16_t* d_sport, void* d_workspace, void* stream) {
    using namespace udp;
    if (!ports || (need | reject) > 0xFFu || n > 0xFFFFFFFFull || nbatch > 0xFFFFFFFFull) return SCCSUM_EINVAL;
    if (!d_index && n > nbatch) return SCCSUM_EINVAL;
    if (!d_first || !d_workspace || misaligned(d_first, 4) || misaligned(d_workspace, 16)) return SCCSUM_EINVAL;
    if (n != 0) {
        if (!d_order || !d_pay_off || !d_pay_len || !d_src || !d_sport) return SCCSUM_EINVAL;
        if (nbatch != 0 && ((!d_bytes && bytes_len != 0) || !d_off || !d_len || !d_status)) return SCCSUM_EINVAL;
        if (misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_index, 4) || misaligned(d_order, 4) ||
            misaligned(d_pay_off, 8) || misaligned(d_pay_len, 4) || misaligned(d_src, 4) || misaligned(d_sport, 2)) {
            return SCCSUM_EINVAL;
        }
    }
    if (ports->device == kHostOnly) return SCCSUM_ENODEV;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, ports->device);
    if (rc != SCCSUM_OK) return rc;
    const FramesDecode dec{static_cast<const uint8_t*>(d_bytes), bytes_len, d_off, d_len, nbatch, d_status, d_index, n,
                           need, reject, host_address, ports->d_table};
    return run_rx(dec, ports->channels, d_class, d_first, RxOut{d_order, d_pay_off, d_pay_len, d_src, d_sport},
                  d_workspace, st);
}

int sccsum_udp_rx_reasm(const sccsum_gather_desc* d_desc, const uint32_t* d_dgram_first, const uint64_t* d_dgram_off,
                        const uint32_t* d_dgram_len, const uint32_t* d_dgram_head, uint64_t m,
                        const sccsum_frag_rec* d_rec, uint64_t nrec, const uint8_t* d_l4_status, uint32_t need,
                        uint32_t reject, uint32_t host_address, const sccsum_udp_ports* ports, uint8_t* d_class,
                        uint32_t* d_first, uint32_t* d_order, uint32_t* d_pay_len, uint32_t* d_src, uint16_t* d_sport,
                        void* d_workspace, void* stream) {
    using namespace udp;
    if (!ports || (need | reject) > 0xFFu || m > 0x7FFFFFFFull || nrec > 0x7FFFFFFFull) return SCCSUM_EINVAL;
    if (!d_l4_status && (need != 0 || reject != 0)) return SCCSUM_EINVAL;
    if (!d_first || !d_workspace || misaligned(d_first, 4) || misaligned(d_workspace, 16)) return SCCSUM_EINVAL;
    if (m != 0) {
        if (!d_desc || !d_dgram_first || !d_dgram_off || !d_dgram_len || !d_dgram_head || (!d_rec && nrec != 0) ||
            !d_order || !d_pay_len || !d_src || !d_sport) {
            return SCCSUM_EINVAL;
        }
        if (misaligned(d_desc, 8) || misaligned(d_dgram_first, 4) || misaligned(d_dgram_off, 8) ||
            misaligned(d_dgram_len, 4) || misaligned(d_dgram_head, 4) || misaligned(d_rec, 8) ||
            misaligned(d_order, 4) || misaligned(d_pay_len, 4) || misaligned(d_src, 4) || misaligned(d_sport, 2)) {
            return SCCSUM_EINVAL;
        }
    }
    if (ports->device == kHostOnly) return SCCSUM_ENODEV;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, ports->device);
    if (rc != SCCSUM_OK) return rc;
    const ReasmDecode dec{d_desc, d_dgram_first, d_dgram_off, d_dgram_len, d_dgram_head, m, d_rec, nrec, d_l4_status,
                          need, reject, host_address, ports->d_table};
    return run_rx(dec, ports->channels, d_class, d_first, RxOut{d_order, nullptr, d_pay_len, d_src, d_sport},
                  d_workspace, st);
}

int sccsum_udp_send(const sccsum_udp_opts* opts, void* d_bytes, uint64_t bytes_len, const uint64_t* d_off,
                    const uint32_t* d_len, const uint32_t* d_dst, const uint16_t* d_dport, const uint16_t* d_sport,
                    uint64_t n, uint64_t* d_l4_off, uint32_t* d_l4_len, uint32_t* d_sum_len, uint32_t* d_seed,
                    uint8_t* d_proto, uint8_t* d_needs_csum, uint8_t* d_status, void* stream) {
    using namespace udp;
    if (!opts || opts->mtu < 68 || opts->mtu > 65535) return SCCSUM_EINVAL;
    if (opts->flags & ~uint32_t(SCCSUM_UDP_CSUM_OFFLOAD | SCCSUM_UDP_UFO)) return SCCSUM_EINVAL;
    if (n > 0xFFFFFFFFull) return SCCSUM_EINVAL;
    if (n != 0) {
        if ((!d_bytes && bytes_len != 0) || !d_off || !d_len || !d_dst || !d_dport || !d_sport || !d_l4_off ||
            !d_l4_len || !d_sum_len || !d_seed || !d_needs_csum || !d_status) {
            return SCCSUM_EINVAL;
        }
        if (misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_dst, 4) || misaligned(d_dport, 2) ||
            misaligned(d_sport, 2) || misaligned(d_l4_off, 8) || misaligned(d_l4_len, 4) || misaligned(d_sum_len, 4) ||
            misaligned(d_seed, 4)) {
            return SCCSUM_EINVAL;
        }
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, -1);
    if (rc != SCCSUM_OK || n == 0) return rc;
    const Send S{static_cast<uint8_t*>(d_bytes), bytes_len, d_off, d_len, d_dst, d_dport, d_sport, n,
                 opts->src_host, opts->mtu, opts->flags};
    const SendOut O{d_l4_off, d_l4_len, d_sum_len, d_seed, d_proto, d_needs_csum, d_status};
    const uint64_t blocks = (n + kSendBlock - 1) / kSendBlock;
    Chain c{st};
    c.launch(send_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kSendBlock), 0, S, O);
    return c.rc();
}

}  // extern "C"
