// send.hip — ipv4::send for a batch on the GPU: the IPv4 header the reference
// prepends to every L4 datagram and the fragmentation loop it runs for one that
// does not fit the MTU (sccsum.h, "Tx send").
//
// What it restates from the reference (paths relative to the reference tree):
//   ipv4::needs_frag      src/net/ip.cc:100-111
//   ipv4::send            src/net/ip.cc:244-299 (the header: 249-281, the cut: 283-294)
//
// No payload byte moves: per wire frame the kernels write one 20-byte header
// and two sccsum_gather_desc records (the header, then the piece of the
// datagram where it lies), the shape p.share(offset, can_send) + prepend has
// in the reference.  The fragment offset is offset / 8 TRUNCATED, as the
// reference computes it: with mtu - 20 not a multiple of 8 the offsets are the
// reference's, not RFC 791's (a receiver would reassemble such pieces wrongly;
// real MTUs minus 20 are multiples of 8 or the datagrams fit).
//
// Four dependent launches on the caller's stream, no block ever waiting on
// another one and no atomic deciding a position (the only atomics are LDS
// minima, whose result does not depend on their order):
//   send_count_kernel   one block per tile of kSendTile datagrams: frames and
//                       layout bytes of every datagram, the tile's totals ->
//                       workspace
//   send_scan_kernel    ONE block: exclusive scan over the tiles (in place),
//                       the totals, and the capacity cutoff: the tile the caps
//                       fall in is scanned again to find the first datagram
//                       that does not fit -> d_total, the closing entries
//   send_place_kernel   one block per tile: the tile's own scan on top of its
//                       base -> d_dgram_first, each datagram's first byte
//                       (workspace), d_status, the SCCSUM_SEND_L4 stores
//   send_emit_kernel    parallel over FRAMES, consecutive lanes consecutive
//                       frames: a frame finds its datagram by binary search in
//                       d_dgram_first (the tile's entries copied to LDS when
//                       they fit), then writes its header, descriptors,
//                       d_first, d_out_off and d_out_len entries
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "host_launch.h"
#include "sccsum.h"
#include "sccsum_diag.h"
#include "wave_scan.h"
#include "wire.h"

namespace send {

using host_launch::Chain;
using host_launch::misaligned;
using host_launch::stream_ok;
using wire::tiles_of;

constexpr int kWave = 64;
constexpr int kTileBlock = 1024;                // threads of the count / scan / place kernels: one datagram each
constexpr int kTileWaves = kTileBlock / kWave;
constexpr uint32_t kSendTile = kTileBlock;      // datagrams per tile
constexpr int kEmitBlock = 256;
constexpr int kEmitRounds = 4;                  // round r of a tile is its frames [256 r, 256 r + 256)
constexpr uint32_t kEmitTile = kEmitBlock * kEmitRounds;
constexpr uint32_t kEmitStage = 2048;          // d_dgram_first entries an emit tile searches in LDS
constexpr uint32_t kEmitMaxBlocks = 16384;      // the emit grid strides over the tiles past this
constexpr uint32_t kIpHdr = 20;
constexpr uint32_t kL4Max = 65535u - kIpHdr;    // ip_packet_len_max - sizeof(ip_hdr)
constexpr uint32_t kKnownFlags = SCCSUM_SEND_TSO | SCCSUM_SEND_UFO | SCCSUM_SEND_NO_IP_CSUM | SCCSUM_SEND_L4;
constexpr uint64_t kNoCut = ~uint64_t(0);

// Workspace: [0] frames emitted, [1] datagrams emitted (the prefix), then per
// tile {frames, bytes} (totals, then their exclusive scan), then every
// datagram's first byte in the packed layout.
constexpr uint64_t kWsHead = 2;

__host__ __device__ inline bool needs_frag(uint32_t len, uint32_t proto, uint32_t mtu, uint32_t flags) {
    if (len + kIpHdr <= mtu) return false;
    if (proto == 6 && (flags & SCCSUM_SEND_TSO)) return false;
    if (proto == 17 && (flags & SCCSUM_SEND_UFO)) return false;
    return true;
}

// Frames ipv4::send makes of a datagram of len <= kL4Max bytes; the layout
// bytes are len + 20 * frames.
__host__ __device__ inline uint32_t frames_of(uint32_t len, uint32_t proto, uint32_t mtu, uint32_t flags) {
    if (!needs_frag(len, proto, mtu, flags)) return 1;
    const uint32_t room = mtu - kIpHdr;
    return (len + room - 1) / room;
}

__host__ __device__ inline bool opts_ok(const sccsum_send_opts& o) {
    return o.mtu >= 68 && o.mtu <= 65535 && (o.flags & ~kKnownFlags) == 0;
}

struct Batch {
    const uint64_t* off;
    const uint32_t* len;
    const uint8_t* proto;
    uint64_t l4_bytes_len;
    uint64_t n;
    uint32_t mtu;
    uint32_t flags;
};

// One datagram's refusal bits (0 = taken) and its count packed as
// frames << 32 | bytes: a tile has at most 1024 * 1366 frames and
// 1024 * 92 835 bytes, so the halves never carry into each other.
__device__ __forceinline__ uint64_t count_one(const Batch& B, uint64_t i, uint32_t* refused) {
    *refused = 0;
    if (i >= B.n) return 0;
    const uint64_t off = B.off[i];
    const uint32_t len = B.len[i];
    uint32_t bad = 0;
    if (off > B.l4_bytes_len || len > B.l4_bytes_len - off) bad |= SCCSUM_ST_RANGE;
    if (len > kL4Max) bad |= SCCSUM_ST_MALFORMED;
    *refused = bad;
    if (bad) return 0;
    const uint32_t frames = frames_of(len, B.proto[i], B.mtu, B.flags);
    return (uint64_t(frames) << 32) | (len + kIpHdr * frames);
}

// Inclusive scan over the 1024 threads of a block; *total = the block's sum.
// `part` is LDS for one value per wave; the call may be repeated.
__device__ __forceinline__ uint64_t block_inclusive_scan(uint64_t v, uint64_t* part, uint64_t* total) {
    return wave_scan::block_inclusive_scan<kTileWaves>(v, part, total);
}

__global__ __launch_bounds__(kTileBlock) void send_count_kernel(Batch B, uint64_t* __restrict__ ws) {
    __shared__ uint64_t part[kTileWaves];
    uint32_t refused;
    const uint64_t c = count_one(B, uint64_t(blockIdx.x) * kSendTile + threadIdx.x, &refused);
    uint64_t total;
    (void)block_inclusive_scan(c, part, &total);
    if (threadIdx.x == 0) {
        ws[kWsHead + 2 * uint64_t(blockIdx.x)] = total >> 32;
        ws[kWsHead + 2 * uint64_t(blockIdx.x) + 1] = total & 0xFFFFFFFFu;
    }
}

__global__ __launch_bounds__(kTileBlock) void send_scan_kernel(Batch B, uint64_t* __restrict__ ws, uint64_t ntiles,
                                                               uint64_t max_frames, uint64_t max_out_bytes,
                                                               uint32_t* __restrict__ d_first,
                                                               uint32_t* __restrict__ d_dgram_first,
                                                               uint64_t* __restrict__ d_total) {
    __shared__ uint64_t part[kTileWaves];
    __shared__ unsigned long long cut_tile;  // the first tile past which a cap is exceeded
    __shared__ unsigned int cut_slot;        // the first datagram of that tile that does not fit
    if (threadIdx.x == 0) {
        cut_tile = kNoCut;
        cut_slot = kSendTile;
    }
    __syncthreads();
    uint64_t frames = 0, bytes = 0;  // carried over the chunks of 1024 tiles
    for (uint64_t base = 0; base < ntiles; base += kTileBlock) {
        const uint64_t t = base + threadIdx.x;
        const uint64_t f = t < ntiles ? ws[kWsHead + 2 * t] : 0;
        const uint64_t b = t < ntiles ? ws[kWsHead + 2 * t + 1] : 0;
        uint64_t fsum, bsum;
        const uint64_t fi = frames + block_inclusive_scan(f, part, &fsum);
        const uint64_t bi = bytes + block_inclusive_scan(b, part, &bsum);
        if (t < ntiles) {
            ws[kWsHead + 2 * t] = fi - f;
            ws[kWsHead + 2 * t + 1] = bi - b;
            if (fi > max_frames || bi > max_out_bytes) atomicMin(&cut_tile, static_cast<unsigned long long>(t));
        }
        frames += fsum;
        bytes += bsum;
    }
    __syncthreads();
    const uint64_t tc = cut_tile;
    uint64_t prefix = B.n, emitted = frames;
    if (tc != kNoCut) {
        // the caps fall inside tile tc: its datagrams once more, on top of its base
        const uint64_t fbase = ws[kWsHead + 2 * tc], bbase = ws[kWsHead + 2 * tc + 1];
        uint32_t refused;
        const uint64_t c = count_one(B, tc * kSendTile + threadIdx.x, &refused);
        uint64_t total;
        const uint64_t incl = block_inclusive_scan(c, part, &total);
        const bool fits = fbase + (incl >> 32) <= max_frames && bbase + (incl & 0xFFFFFFFFu) <= max_out_bytes;
        if (!fits) atomicMin(&cut_slot, threadIdx.x);
        __syncthreads();
        const uint32_t k = cut_slot;  // < kSendTile: the tile's total does not fit
        __shared__ uint64_t at_cut;
        if (threadIdx.x == k) at_cut = fbase + ((incl - c) >> 32);
        __syncthreads();
        prefix = tc * kSendTile + k;
        emitted = at_cut;
    }
    if (threadIdx.x == 0) {
        ws[0] = emitted;
        ws[1] = prefix;
        d_total[0] = frames;
        d_total[1] = bytes;
        d_total[2] = prefix;
        d_dgram_first[B.n] = static_cast<uint32_t>(emitted);
        if (d_first) d_first[emitted] = static_cast<uint32_t>(2 * emitted);  // the closing entry
    }
}

__global__ __launch_bounds__(kTileBlock) void send_place_kernel(Batch B, uint64_t* __restrict__ ws, uint64_t ntiles,
                                                                uint8_t* __restrict__ d_l4,
                                                                const uint16_t* __restrict__ d_l4sum,
                                                                uint32_t* __restrict__ d_dgram_first,
                                                                uint8_t* __restrict__ d_status) {
    __shared__ uint64_t part[kTileWaves];
    const uint64_t emitted = ws[0], prefix = ws[1];
    const uint64_t i = uint64_t(blockIdx.x) * kSendTile + threadIdx.x;
    uint32_t refused;
    const uint64_t c = count_one(B, i, &refused);
    uint64_t total;
    const uint64_t excl = block_inclusive_scan(c, part, &total) - c;
    if (i >= B.n) return;
    const uint64_t first_frame = ws[kWsHead + 2 * uint64_t(blockIdx.x)] + (excl >> 32);
    const uint64_t first_byte = ws[kWsHead + 2 * uint64_t(blockIdx.x) + 1] + (excl & 0xFFFFFFFFu);
    const bool in_prefix = i < prefix;
    d_dgram_first[i] = static_cast<uint32_t>(in_prefix ? first_frame : emitted);
    ws[kWsHead + 2 * ntiles + i] = first_byte;
    d_status[i] = static_cast<uint8_t>(!in_prefix ? 0u : refused ? refused : SCCSUM_ST_OK);
    if (d_l4sum && in_prefix && !refused) {
        const uint32_t len = B.len[i];
        const uint32_t proto = B.proto[i];
        uint32_t at = 0;
        if (proto == 17 && len >= 8) at = 6;
        if (proto == 6 && len >= 20) at = 16;
        if (at) {
            // the value's bytes are the wire bytes, at any alignment
            const uint16_t v = d_l4sum[i];
            uint8_t* const p = d_l4 + B.off[i] + at;
            p[0] = static_cast<uint8_t>(v & 0xFF);
            p[1] = static_cast<uint8_t>(v >> 8);
        }
    }
}

struct Out {
    uint8_t* hdr;
    sccsum_gather_desc* desc;
    uint32_t* first;
    uint64_t* out_off;
    uint32_t* out_len;
};

// RFC 1071 over the ten 16-bit words of the header with a zero field, from the
// fields themselves; the value as the big-endian word at +10.
__device__ __forceinline__ uint32_t header_csum(uint32_t total_len, uint32_t id, uint32_t frag, uint32_t proto,
                                                uint32_t src, uint32_t dst) {
    uint32_t s = 0x4500u + total_len + id + frag + ((64u << 8) | proto) + (src >> 16) + (src & 0xFFFFu) + (dst >> 16) +
                 (dst & 0xFFFFu);
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return ~s & 0xFFFFu;
}

__device__ __forceinline__ uint32_t be16(uint32_t v) { return ((v & 0xFFu) << 8) | ((v >> 8) & 0xFFu); }
__device__ __forceinline__ uint32_t be32(uint32_t v) { return __builtin_bswap32(v); }

__global__ __launch_bounds__(kEmitBlock) void send_emit_kernel(Batch B, const uint64_t* __restrict__ ws, uint64_t ntiles,
                                                               const uint8_t* __restrict__ d_l4,
                                                               const uint32_t* __restrict__ d_dst,
                                                               const uint16_t* __restrict__ d_id,
                                                               const uint32_t* __restrict__ d_dgram_first,
                                                               uint32_t src_host, Out O) {
    __shared__ uint64_t range[2];        // the datagrams of the tile's first and last frame
    __shared__ uint32_t staged[kEmitStage];  // their d_dgram_first entries, when they fit
    const uint64_t emitted = ws[0], prefix = ws[1];
    const uint64_t* const first_byte = ws + kWsHead + 2 * ntiles;
    const uint32_t room = B.mtu - kIpHdr;
    const bool hdr_words = (reinterpret_cast<uintptr_t>(O.hdr) & 3u) == 0;  // then every header is 4-byte aligned
    // the last datagram d in [lo, hi) with first(d) <= f, given first(lo) <= f < first(hi)
    auto owner = [](auto first, uint64_t f, uint64_t lo, uint64_t hi) {
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (first(mid) <= f) lo = mid; else hi = mid;
        }
        return lo;
    };
    const auto global_first = [&](uint64_t d) { return d_dgram_first[d]; };
    for (uint64_t f0 = uint64_t(blockIdx.x) * kEmitTile; f0 < emitted; f0 += uint64_t(gridDim.x) * kEmitTile) {
        const uint64_t last = (emitted - f0 < kEmitTile ? emitted : f0 + kEmitTile) - 1;
        __syncthreads();  // the last tile's readers are done with range and staged
        if (threadIdx.x == 0) range[0] = owner(global_first, f0, 0, prefix);
        if (threadIdx.x == kWave) range[1] = owner(global_first, last, 0, prefix);
        __syncthreads();
        // the tile's frames belong to datagrams lo .. hi - 1: at most 1024 that have frames, and the
        // frameless ones between them
        const uint64_t lo = range[0], hi = range[1] + 1;
        const bool in_lds = hi - lo <= kEmitStage;
        if (in_lds) {
            for (uint32_t j = threadIdx.x; j < hi - lo; j += kEmitBlock) staged[j] = d_dgram_first[lo + j];
        }
        __syncthreads();
        const auto staged_first = [&](uint64_t d) { return staged[d - lo]; };
#pragma unroll
        for (int r = 0; r < kEmitRounds; ++r) {
            const uint64_t f = f0 + uint64_t(r) * kEmitBlock + threadIdx.x;
            if (f > last) continue;
            const uint64_t i = in_lds ? owner(staged_first, f, lo, hi) : owner(global_first, f, lo, hi);
            const uint32_t k = static_cast<uint32_t>(f - (in_lds ? staged[i - lo] : d_dgram_first[i]));
            const uint32_t len = B.len[i];
            const uint32_t proto = B.proto[i];
            const bool cut = needs_frag(len, proto, B.mtu, B.flags);
            const uint32_t o = cut ? k * room : 0u;
            if (cut && o >= len) continue;  // never: k is below the datagram's frame count
            const uint32_t piece = !cut ? len : len - o < room ? len - o : room;
            const uint32_t frag = cut ? ((o + piece < len ? 0x2000u : 0u) | (o >> 3)) : 0u;
            const uint32_t total_len = kIpHdr + piece;
            const uint32_t id = d_id ? d_id[i] : 0u;
            const uint32_t dst = d_dst[i];
            const uint32_t csum =
                (B.flags & SCCSUM_SEND_NO_IP_CSUM) ? 0u : header_csum(total_len, id, frag, proto, src_host, dst);
            const uint64_t at = first_byte[i] + uint64_t(k) * (room + kIpHdr);  // the pieces before it are full

            const uint32_t h[5] = {0x45u | (be16(total_len) << 16), be16(id) | (be16(frag) << 16),
                                   64u | (proto << 8) | (be16(csum) << 16), be32(src_host), be32(dst)};
            uint8_t* const hp = O.hdr + f * kIpHdr;
            if (hdr_words) {
#pragma unroll
                for (int w = 0; w < 5; ++w) reinterpret_cast<uint32_t*>(hp)[w] = h[w];
            } else {  // d_hdr at an odd address: the same bytes one at a time
#pragma unroll
                for (int b = 0; b < 20; ++b) hp[b] = static_cast<uint8_t>(h[b / 4] >> (8 * (b % 4)));
            }
            const uint32_t at32 = static_cast<uint32_t>(at);
            uint64_t* const d = reinterpret_cast<uint64_t*>(O.desc + 2 * f);
            d[0] = reinterpret_cast<uint64_t>(O.hdr + f * kIpHdr);
            d[1] = uint64_t(at32) | (uint64_t(kIpHdr) << 32);
            d[2] = reinterpret_cast<uint64_t>(d_l4 + B.off[i] + o);
            d[3] = uint64_t(at32 + kIpHdr) | (uint64_t(piece) << 32);
            O.first[f] = static_cast<uint32_t>(2 * f);
            O.out_off[f] = at;
            O.out_len[f] = total_len;
        }
    }
}

// ---------------------------------------------------------------- host side

static_assert(sizeof(sccsum_gather_desc) == 16 && offsetof(sccsum_gather_desc, dst_off) == 8 &&
                  offsetof(sccsum_gather_desc, len) == 12,
              "the emit kernel stores a descriptor as two 64-bit words");

}  // namespace send

extern "C" {

int sccsum_send_tile_datagrams(void) { return static_cast<int>(send::kSendTile); }
int sccsum_send_emit_tile_frames(void) { return static_cast<int>(send::kEmitTile); }

int sccsum_ipv4_send_plan(const sccsum_send_opts* opts, uint32_t l4_len, uint8_t proto, uint32_t* nframes,
                          uint64_t* out_bytes) {
    if (nframes) *nframes = 0;
    if (out_bytes) *out_bytes = 0;
    if (!opts || !nframes || !out_bytes || !send::opts_ok(*opts)) return SCCSUM_EINVAL;
    if (l4_len > send::kL4Max) return SCCSUM_OK;  // refused: SCCSUM_ST_MALFORMED, no frame
    const uint32_t frames = send::frames_of(l4_len, proto, opts->mtu, opts->flags);
    *nframes = frames;
    *out_bytes = uint64_t(l4_len) + uint64_t(send::kIpHdr) * frames;
    return SCCSUM_OK;
}

uint64_t sccsum_ipv4_send_workspace(uint64_t n) {
    const uint64_t words = send::kWsHead + 2 * send::tiles_of(n, send::kSendTile) + n;
    return (words * 8 + 15) & ~uint64_t(15);
}

int sccsum_ipv4_send(const sccsum_send_opts* opts, void* d_l4, uint64_t l4_bytes_len, const uint64_t* d_off,
                     const uint32_t* d_len, const uint32_t* d_dst, const uint8_t* d_proto, const uint16_t* d_id,
                     const uint16_t* d_l4sum, uint64_t n, uint64_t max_frames, uint64_t max_out_bytes, uint8_t* d_hdr,
                     sccsum_gather_desc* d_desc, uint32_t* d_first, uint64_t* d_out_off, uint32_t* d_out_len,
                     uint32_t* d_dgram_first, uint8_t* d_status, uint64_t* d_total, void* d_workspace, void* stream) {
    using namespace send;
    if (!opts || !opts_ok(*opts)) return SCCSUM_EINVAL;
    if (max_frames > 0x7FFFFFFFull || max_out_bytes > 0xFFFFFFFFull || n > 0xFFFFFFFFull) return SCCSUM_EINVAL;
    if (((opts->flags & SCCSUM_SEND_L4) != 0) != (d_l4sum != nullptr) && n != 0) return SCCSUM_EINVAL;
    if (n == 0 && d_l4sum && !(opts->flags & SCCSUM_SEND_L4)) return SCCSUM_EINVAL;
    if (!d_total || !d_dgram_first || !d_workspace) return SCCSUM_EINVAL;
    if (misaligned(d_total, 8) || misaligned(d_dgram_first, 4) || misaligned(d_workspace, 16) ||
        misaligned(d_first, 4)) {
        return SCCSUM_EINVAL;
    }
    if (n != 0) {
        if ((!d_l4 && l4_bytes_len != 0) || !d_off || !d_len || !d_dst || !d_proto || !d_status || !d_hdr || !d_desc ||
            !d_first || !d_out_off || !d_out_len) {
            return SCCSUM_EINVAL;
        }
        if (misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_dst, 4) || misaligned(d_id, 2) ||
            misaligned(d_l4sum, 2) || misaligned(d_desc, 8) || misaligned(d_out_off, 8) ||
            misaligned(d_out_len, 4)) {
            return SCCSUM_EINVAL;
        }
    }
    // the launches run on the stream's device, which must be the data's: the current one
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, -1);
    if (rc != SCCSUM_OK) return rc;

    const Batch B{d_off, d_len, d_proto, l4_bytes_len, n, opts->mtu, opts->flags};
    const uint64_t ntiles = tiles_of(n, kSendTile);
    uint64_t* const ws = static_cast<uint64_t*>(d_workspace);
    const dim3 tiles(static_cast<unsigned>(ntiles)), block(kTileBlock);
    Chain c{st};
    if (ntiles) c.launch(send_count_kernel, tiles, block, 0, B, ws);
    c.launch(send_scan_kernel, dim3(1), block, 0, B, ws, ntiles, max_frames, max_out_bytes, d_first, d_dgram_first,
             d_total);
    if (!ntiles) return c.rc();
    c.launch(send_place_kernel, tiles, block, 0, B, ws, ntiles, d_l4, d_l4sum, d_dgram_first, d_status);
    if (max_frames == 0) return c.rc();
    const uint64_t blocks = std::min<uint64_t>((max_frames + kEmitTile - 1) / kEmitTile, kEmitMaxBlocks);
    const Out O{d_hdr, d_desc, d_first, d_out_off, d_out_len};
    c.launch(send_emit_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kEmitBlock), 0, B, ws, ntiles, d_l4, d_dst, d_id,
             d_dgram_first, opts->src_host, O);
    return c.rc();
}

}  // extern "C"
