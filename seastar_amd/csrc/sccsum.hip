// sccsum.hip — CDNA4 (gfx950) batch Internet checksum kernels and the C-ABI
// launchers declared in include/sccsum.h.
//
// Arithmetic (see DESIGN.md "Arithmetic domain"): the reference adds
// big-endian 16-bit words into an __int128 and returns htons(~fold(S))
// (src/net/ip_checksum.cc:31-62).  Because 2^16 == 1 (mod 65535) and
// byte-swapping a 16-bit word multiplies it by 256 (mod 65535), the same
// uint16_t comes out of: sum the bytes as LITTLE-endian 32-bit words, fold
// with end-around carry (zero stays zero, nonzero stays nonzero), byte-swap if
// the span starts at an odd address, complement.  So the kernel may group,
// reorder and widen freely — it loads aligned 16-byte units.
//
// Layout: packets live anywhere inside one byte buffer behind an
// offset (u64) / length (u32) array.  Default kernel (csum_flat_kernel): a
// wavefront takes a tile of up to 64 packets (one per lane), splits it into
// runs of packets that lie forward in memory, streams each run's 16-byte units
// densely through one raw buffer descriptor (nt loads), sums every unit with
// v_sad_u16, prefix-scans the unit sums across the wave (DPP) and lets each
// packet lane pick up the two prefix values that bound its units; each lane
// then finishes its packet (edge-byte correction, IPv4 header decode,
// pseudo-header, complement) with one coalesced store per tile.  No MFMA: a
// byte reduction at the HBM read roofline.  csum_kernel is a deliberately
// plain second implementation (one packet per wave, per-lane byte masks) kept
// for cross-checking.

#include <hip/hip_runtime.h>
#include "engine_seal.h"

#include <atomic>
#include <cctype>
#include <chrono>
#include <cstring>
#include <new>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <vector>

#include "host_launch.h"
#include "sccsum.h"
#include "sccsum_diag.h"

namespace sccsum {
namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kBlocksPerCU = 8;  // 32 waves/CU: needs <= 64 VGPRs
constexpr int kMaxDevices = 64;
constexpr uint32_t kFlagRaw = 1;     // spans: output the folded span-relative sum (no seed, no complement)
constexpr uint32_t kFlagFillL4 = 2;  // frames: generate the TCP/UDP checksum and store it in the frame
constexpr uint32_t kFlagFillIp = 4;  // frames (with kFlagFillL4): also generate + store the IPv4 header checksum
constexpr uint32_t kFlagFillIcmp = 8;  // frames: turn ICMP echo requests into replies in place (ip.cc:464-474)
constexpr uint32_t kFillFlags = kFlagFillL4 | kFlagFillIcmp;  // the in-place (FILL) instantiation
constexpr uint32_t kFlagFillNow = 64;  // frames (FILL): each tile stores its frames' fields itself (one pass)
constexpr uint32_t kFlagFullChunks = 16;  // flat kernel: a run's last chunk loads all U rows (diagnostic A/B)
constexpr uint32_t kFlagEngineWT = 32;    // engine: results written through (sc0 sc1), else stored by the launch
                                          // rule and released (agent scope) before a step's count
constexpr uint32_t kRunAlignShift = 12;   // flat kernel, flags bits 12-13: run extents start on 1 / 4 / 8-unit boundaries

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- device helpers

// End-around-carry fold of a 64-bit sum to [0, 0xffff]; 0 iff s == 0.
__device__ __forceinline__ uint32_t fold16(uint64_t s) {
    s = (s & 0xffffffffull) + (s >> 32);
    s = (s & 0xffffull) + (s >> 16);
    s = (s & 0xffffull) + (s >> 16);
    s = (s & 0xffffull) + (s >> 16);
    return static_cast<uint32_t>(s);
}

__device__ __forceinline__ uint32_t swap16(uint32_t x) {
    return ((x & 0xffu) << 8) | (x >> 8);
}

// Keep the bytes of dword `d` (bytes 4d..4d+3 of a 16-byte unit) that fall in
// [lo, hi) (unit-relative, may be out of [0,16]).
__device__ __forceinline__ uint32_t keep_bytes(uint32_t w, int lo, int hi, int d) {
    const int a = min(max(lo - 4 * d, 0), 4);
    const int b = min(max(hi - 4 * d, 0), 4);
    const uint64_t m = ((1ull << (8 * b)) - 1ull) & ~((1ull << (8 * a)) - 1ull);
    return w & static_cast<uint32_t>(m);
}

__device__ __forceinline__ uint64_t unit_sum(const u32x4& v, int lo, int hi) {
    uint64_t s = keep_bytes(v.x, lo, hi, 0);
    s += keep_bytes(v.y, lo, hi, 1);
    s += keep_bytes(v.z, lo, hi, 2);
    s += keep_bytes(v.w, lo, hi, 3);
    return s;
}

// Sum of a 32-bit value over the 64 lanes of the wave.  All lanes must be
// active.  quad_perm xor1/xor2 and row_ror 4/8 give every lane its 16-lane
// row total; four readlanes add the rows.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0xB1, 0xF, 0xF, false));
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x4E, 0xF, 0xF, false));
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x124, 0xF, 0xF, false));
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x128, 0xF, 0xF, false));
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 0)) +
           static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 16)) +
           static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 32)) +
           static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 48));
}

// Global (address space 1) views of device pointers.  A pointer the compiler
// cannot place — one read from memory or made from an integer, like the
// engine's descriptor fields — would otherwise be accessed as FLAT, and one
// FLAT access in flight makes every later wait a full vmcnt(0): a chunk then
// waits for all of its loads before summing the first (measured: the engine
// ran 15 % slower than a launch until its pointers were cast, profiles/r04j).
#define SCCSUM_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ const SCCSUM_GLOBAL T* gld(const T* p) {
    return (const SCCSUM_GLOBAL T*)p;
}
template <typename T>
__device__ __forceinline__ SCCSUM_GLOBAL T* gst(T* p) {
    return (SCCSUM_GLOBAL T*)p;
}

__device__ __forceinline__ u32x4 load_unit(const uint8_t* p) {
    return __builtin_nontemporal_load(gld(reinterpret_cast<const u32x4*>(p)));
}

// Logical block id with XCD affinity: blocks b, b+8, b+16 ... are dealt to one
// XCD, so give them consecutive logical ids; neighbouring packets (which share
// their boundary 16-byte unit / cache line) then land on one XCD's L2.
__device__ __forceinline__ uint32_t xcd_block_id() {
    const uint32_t g = gridDim.x;  // host keeps it a multiple of 8
    const uint32_t b = blockIdx.x;
    return (b & 7u) * (g >> 3) + (b >> 3);
}

// ---------------------------------------------------------------- kernels

// The rx path's decode of an IPv4 frame of L bytes from its first 20 bytes as
// little-endian dwords h0..h4 (ipv4::handle_received_packet, ip.cc:114-229):
// the length checks (drop when shorter than the IP length, :137-139; when the
// fragment offset + datagram length passes 65 535, :141-144; a 4*ihl strip
// past the datagram), the fragment test (MF set or offset != 0, ip.hh:400-402,
// ip.cc:165-166), the L4 range [l4_off, l4_off + l4_len) (the IP total length
// clipped to the frame) and the L4 seed: the TCP / UDP pseudo-header
// (ip.hh:70-75) in the little-endian domain — the address words are dwords 3
// and 4, then (0, proto) and the big-endian L4 length byte-swapped — and none
// for ICMP (ip.cc:471-474) or any other protocol.
struct FrameDecode {
    uint32_t ihl, ip_len, proto, l4_off, l4_len, pseudo;
    uint32_t st;  // SCCSUM_ST_MALFORMED / SCCSUM_ST_IPFRAG
};

__device__ __forceinline__ FrameDecode frame_decode(uint32_t h0, uint32_t h1, uint32_t h2, uint32_t h3, uint32_t h4,
                                                    uint32_t L) {
    FrameDecode D{};
    D.ihl = h0 & 0xfu;
    D.ip_len = swap16(h0 >> 16);
    D.proto = (h2 >> 8) & 0xffu;
    D.l4_off = 4u * D.ihl;
    const uint32_t l4_end = D.ip_len < L ? D.ip_len : L;
    const uint32_t fragw = swap16(h1 >> 16);  // flags + fragment offset (ip.hh:388-389)
    if (L < D.ip_len || (fragw & 0x1fffu) * 8u + l4_end > 65535u) D.st |= SCCSUM_ST_MALFORMED;
    if (fragw & 0x3fffu) D.st |= SCCSUM_ST_IPFRAG;
    if (D.l4_off > l4_end) {
        D.st |= SCCSUM_ST_MALFORMED;
    } else {
        D.l4_len = l4_end - D.l4_off;
    }
    const bool tcp_udp = D.proto == 6u || D.proto == 17u;
    D.pseudo = tcp_udp ? fold16(static_cast<uint64_t>(h3 & 0xffffu) + (h3 >> 16) + (h4 & 0xffffu) + (h4 >> 16) +
                                (D.proto << 8) + swap16(D.l4_len & 0xffffu))
                       : 0u;
    return D;
}

// A frame's result word (IP | L4 << 16) and status from its header checksum,
// its L4 result r and the decode's bits: an IP fragment claims no L4 value
// (the reference sums L4 over the reassembled datagram only, ip.cc:164-220).
__device__ __forceinline__ uint32_t frame_word(uint32_t ipc, uint32_t r, uint32_t st) {
    return ipc | ((st & SCCSUM_ST_IPFRAG) ? 0u : r << 16);
}
__device__ __forceinline__ uint32_t frame_status(uint32_t ipc, uint32_t r, uint32_t st) {
    return st | (ipc == 0 ? SCCSUM_ST_OK : 0u) | ((st & SCCSUM_ST_IPFRAG) == 0u && r == 0 ? SCCSUM_ST_L4_OK : 0u);
}

struct FrameHeader {
    uint32_t ipc, l4_off, l4_len, pseudo;
    uint8_t st;
};

__device__ __forceinline__ FrameHeader frame_header(uint32_t h0, uint32_t h1, uint32_t h2, uint32_t h3, uint32_t h4,
                                                    uint32_t L) {
    FrameHeader F{};
    F.ipc = ~fold16(static_cast<uint64_t>(h0) + h1 + h2 + h3 + h4) & 0xffffu;
    const FrameDecode D = frame_decode(h0, h1, h2, h3, h4, L);
    F.l4_off = D.l4_off;
    F.l4_len = D.l4_len;
    F.pseudo = D.pseudo;
    F.st = static_cast<uint8_t>(D.st);
    return F;
}

// One contiguous packet of L bytes at ptr, summed by one wave: U 16-byte
// units per lane in flight; frame mode reads the IPv4 header with the first
// units (one round trip) and sums the L4 range only.  S is the folded sum of
// the summed range at its packet parity (byte-swapped back when ptr is odd),
// before the pseudo-header / seed.
struct PacketSum {
    uint32_t S, ipc, pseudo;
    uint8_t st;
};

// span_packet and the fragment loop of csum_desc_kernel carry byte ranges and
// unit indices as int / uint32_t: a span (a fragment) of kWideLen bytes or
// more goes to exact_range_sum, 64-bit throughout, so every uint32_t length
// sums exactly and the common path's arithmetic never leaves [0, 2^31).
constexpr uint32_t kWideLen = 1u << 30;
__device__ uint32_t exact_range_sum(const uint8_t* a0, uint64_t rs, uint64_t re, uint32_t lane);

template <int U, bool IPV4>
__device__ __forceinline__ PacketSum span_packet(const uint8_t* ptr, uint32_t L, int lane) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(ptr);
    const int head = static_cast<int>(addr & 15u);
    const uint8_t* a0 = ptr - head;
    if (!IPV4 && L >= kWideLen) {  // (L is wave-uniform)
        PacketSum W{};
        W.S = exact_range_sum(a0, static_cast<uint64_t>(head), static_cast<uint64_t>(head) + L,
                              static_cast<uint32_t>(lane));
        if (addr & 1u) W.S = swap16(W.S);
        return W;
    }
    // a frame's summed bytes end at min(ip_len, L) <= 65 535, whatever L is:
    // the units past them are never loaded (and head + L + 15 cannot wrap)
    const uint32_t Lu = IPV4 && L > 65535u ? 65535u : L;
    const uint32_t nunits = Lu ? (static_cast<uint32_t>(head) + Lu + 15u) >> 4 : 0u;

    // Frame mode: the 20-byte IPv4 header as 5 dwords re-aligned to the
    // packet start (lanes 0..5 load the covering dwords; lane 5 only when
    // the packet is not 4-byte aligned, so every dword read holds a
    // header byte and stays inside the 16-byte unit bound).
    uint32_t hv = 0;
    const int s = static_cast<int>(addr & 3u);
    if (IPV4) {
        if (lane < 5 || (lane == 5 && s != 0)) {
            hv = *reinterpret_cast<const uint32_t*>(ptr - s + 4 * lane);
        }
    }

    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t c = static_cast<uint32_t>(u * kWave + lane);
        v[u] = c < nunits ? load_unit(a0 + 16u * c) : u32x4{0, 0, 0, 0};
    }

    PacketSum R{};
    int rs = head;  // summed range, relative to a0
    int re = head + static_cast<int>(L);
    if (IPV4) {
        const uint32_t nxt = static_cast<uint32_t>(
            __builtin_amdgcn_update_dpp(0, static_cast<int>(hv), 0x101, 0xF, 0xF, false));  // row_shl:1
        const uint32_t al = __builtin_amdgcn_alignbyte(nxt, hv, static_cast<uint32_t>(s));
        const FrameHeader F = frame_header(
            __builtin_amdgcn_readlane(al, 0), __builtin_amdgcn_readlane(al, 1), __builtin_amdgcn_readlane(al, 2),
            __builtin_amdgcn_readlane(al, 3), __builtin_amdgcn_readlane(al, 4), L);
        R.ipc = F.ipc;
        R.st = F.st;
        R.pseudo = F.pseudo;
        rs = head + static_cast<int>(F.l4_off);
        re = rs + static_cast<int>(F.l4_len);
    }

    uint64_t acc = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c16 = 16 * (u * kWave + lane);
        acc += unit_sum(v[u], rs - c16, re - c16);
    }
    for (uint32_t g = U * kWave; g < nunits; g += U * kWave) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t c = g + static_cast<uint32_t>(u * kWave + lane);
            v[u] = c < nunits ? load_unit(a0 + 16u * c) : u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c16 = 16 * static_cast<int>(g + u * kWave + lane);
            acc += unit_sum(v[u], rs - c16, re - c16);
        }
    }

    R.S = fold16(wave_sum(fold16(acc)));
    if (addr & 1u) R.S = swap16(R.S);  // span starts at an odd address (4*ihl is even)
    return R;
}

// U = 16-byte units in flight per lane per group (packet bytes covered by one
// group = U * 1 KiB).  IPV4 = frame mode (IPv4 header + L4 with pseudo-header).
template <int U, bool IPV4>
__global__ __launch_bounds__(kBlock) void csum_kernel(
    const uint8_t* __restrict__ bytes, uint64_t bytes_len,
    const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
    const uint32_t* __restrict__ seed, uint16_t* __restrict__ out,
    uint8_t* __restrict__ status, uint64_t n, uint32_t flags) {
    const bool raw = !IPV4 && (flags & kFlagRaw);
    const int lane = static_cast<int>(threadIdx.x & (kWave - 1));
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;

    for (uint64_t p = static_cast<uint64_t>(xcd_block_id()) * kWavesPerBlock + wv; p < n; p += stride) {
        const uint64_t o = off[p];
        const uint32_t L = len[p];
        if (o > bytes_len || L > bytes_len - o || (IPV4 && L < 20)) {
            if (lane == 0) {
                if (IPV4) {
                    if (out) reinterpret_cast<uint32_t*>(out)[p] = 0;
                } else {
                    out[p] = 0;
                }
                if (status) {
                    status[p] = (o > bytes_len || L > bytes_len - o) ? SCCSUM_ST_RANGE : SCCSUM_ST_MALFORMED;
                }
            }
            continue;
        }
        const PacketSum R = span_packet<U, IPV4>(bytes + o, L, lane);
        uint32_t S = R.S;
        const uint32_t ipc = R.ipc;
        const uint8_t st = R.st;
        if (IPV4) {
            S = fold16(static_cast<uint64_t>(S) + R.pseudo);
        } else if (seed && !raw) {
            S = fold16(static_cast<uint64_t>(S) + swap16(fold16(seed[p])));
        }
        const uint32_t r = raw ? S : ~S & 0xffffu;
        if (lane == 0) {
            if (IPV4) {
                if (out) reinterpret_cast<uint32_t*>(out)[p] = frame_word(ipc, r, st);
                if (status) status[p] = static_cast<uint8_t>(frame_status(ipc, r, st));
            } else {
                out[p] = static_cast<uint16_t>(r);
                if (status) status[p] = (!raw && r == 0) ? SCCSUM_ST_OK : 0u;
            }
        }
    }
}

// Keep bytes [lo, hi) of a 64-bit half unit (half-relative byte indices).
__device__ __forceinline__ uint64_t keep_half(uint64_t q, int lo, int hi) {
    const int a = min(max(lo, 0), 8);
    const int b = min(max(hi, 0), 8);
    const int w = b - a;
    const int sh = w > 0 ? 64 - 8 * w : 0;
    const uint64_t m = (~0ull >> sh) << (8 * (w > 0 ? a : 0));
    return w > 0 ? (q & m) : 0ull;
}

// Sum the four dwords of a unit as 16-bit halves into a 32-bit accumulator
// (v_sad_u16 with a zero operand: lo16 + hi16 + acc, one instruction per dword).
__device__ __forceinline__ uint32_t sad4(const u32x4& v, uint32_t acc) {
    acc = __builtin_amdgcn_sad_u16(v.x, 0u, acc);
    acc = __builtin_amdgcn_sad_u16(v.y, 0u, acc);
    acc = __builtin_amdgcn_sad_u16(v.z, 0u, acc);
    return __builtin_amdgcn_sad_u16(v.w, 0u, acc);
}

// Masked unit (bytes [lo, hi) kept, unit-relative) summed like sad4.
__device__ __forceinline__ uint32_t sad4_masked(const u32x4& v, int lo, int hi, uint32_t acc) {
    const uint64_t k0 = keep_half(static_cast<uint64_t>(v.x) | (static_cast<uint64_t>(v.y) << 32), lo, hi);
    const uint64_t k1 = keep_half(static_cast<uint64_t>(v.z) | (static_cast<uint64_t>(v.w) << 32), lo - 8, hi - 8);
    acc = __builtin_amdgcn_sad_u16(static_cast<uint32_t>(k0), 0u, acc);
    acc = __builtin_amdgcn_sad_u16(static_cast<uint32_t>(k0 >> 32), 0u, acc);
    acc = __builtin_amdgcn_sad_u16(static_cast<uint32_t>(k1), 0u, acc);
    return __builtin_amdgcn_sad_u16(static_cast<uint32_t>(k1 >> 32), 0u, acc);
}

// Sum of the bytes [lo, hi) of a 16-byte unit as little-endian 16-bit words
// at their unit-relative positions (sad4 of the masked unit).
__device__ __forceinline__ uint32_t unit_part(const u32x4& v, int lo, int hi) {
    return sad4_masked(v, lo, hi, 0u);
}

// Sum of v over each 16-lane row, in every lane of the row (the first four
// steps of wave_sum).  All lanes of a row must be active.
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0xB1, 0xF, 0xF, false));
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x4E, 0xF, 0xF, false));
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x124, 0xF, 0xF, false));
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x128, 0xF, 0xF, false));
    return v;
}


// ---------------------------------------------------------------- flat-kernel helpers

constexpr int kRsrcFlags = 0x00020000;  // raw buffer, 32-bit data format (gfx950)
constexpr int kNT = 2;                  // nontemporal: streamed once

// Descriptor inputs pass through readfirstlane so the compiler can prove the
// descriptor wave-uniform (otherwise it wraps every buffer op in a waterfall
// loop: guide T20).  Callers only pass wave-uniform values.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const uint8_t* base, uint32_t bytes) {
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(b));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(b >> 32));
    const uint32_t nb = __builtin_amdgcn_readfirstlane(bytes);
    void* p = reinterpret_cast<void*>((static_cast<uint64_t>(hi) << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(p, static_cast<short>(0), static_cast<int>(nb), kRsrcFlags);
}

constexpr uint32_t kExactMax = 131072;  // fast path keeps exact 32-bit sums up to this length

// tile-head counters: each on its own 256-byte line (atomics to one line
// serialise at the memory side: ~12 ns each chip-wide)
constexpr uint32_t kHeadStride = 64;                      // uint32 words between counters
constexpr uint32_t kGroups = 64;                            // tile-dequeue counters per launch

// Exact folded sum (little-endian domain relative to a0) of [rs, re), one
// wave, any length: the slow path for packets the flat pass cannot take.
__device__ uint32_t exact_range_sum(const uint8_t* a0, uint64_t rs, uint64_t re, uint32_t lane) {
    uint64_t acc = 0;
    if (re > rs) {
        const uint64_t c0 = rs >> 4, c1 = (re - 1) >> 4;
        for (uint64_t c = c0; c <= c1; c += kWave) {
            const uint64_t cu = c + lane;
            u32x4 w = u32x4{0, 0, 0, 0};
            if (cu <= c1) w = load_unit(a0 + 16 * cu);
            const int64_t lo = static_cast<int64_t>(rs) - static_cast<int64_t>(16 * cu);
            const int64_t hi = static_cast<int64_t>(re) - static_cast<int64_t>(16 * cu);
            const int l = static_cast<int>(lo < -16 ? -16 : (lo > 32 ? 32 : lo));
            const int h = static_cast<int>(hi < -16 ? -16 : (hi > 32 ? 32 : hi));
            acc += sad4_masked(w, l, h, 0u);
        }
    }
    return fold16(wave_sum(fold16(acc)));
}

// ---------------------------------------------------------------- RSS (Toeplitz)

// toeplitz_hash (include/seastar/net/toeplitz.hh:78-98) XORs, for every set
// data bit j (MSB first), the 32-bit key window that starts at key bit j; key
// bits past key_len read as 0.  The host precomputes the 96 windows a 12-byte
// IPv4 forward_hash can touch, so a lane's hash is 96 select-XORs, and a
// datagram without ports hashes its 8 IP bytes by zeroing the port word.
struct RssParams {
    uint32_t* hash;  // per-frame output (nullptr: no RSS)
    uint32_t mode;   // SCCSUM_RSS_DISPATCH / SCCSUM_RSS_REASSEMBLED
    uint32_t w[96];  // key window at data bit j
};

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

__device__ __forceinline__ uint32_t toeplitz96(const RssParams& P, uint32_t d0, uint32_t d1, uint32_t d2) {
    uint32_t h = 0;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        h ^= (d0 & (0x80000000u >> j)) ? P.w[j] : 0u;
        h ^= (d1 & (0x80000000u >> j)) ? P.w[32 + j] : 0u;
        h ^= (d2 & (0x80000000u >> j)) ? P.w[64 + j] : 0u;
    }
    return h;
}

// The forward_hash of one IPv4 frame (net.hh:53-75, bytes in wire order):
// h0..h4 = the header's dwords as loaded (little-endian), ports20 = the dword
// at frame byte 20, ports_l4 = the dword at 4*ihl (REASSEMBLED only).
//  DISPATCH (net.cc:330-341 -> ip.cc:77-92): src, dst; then for an atomic
//    datagram (MF clear, offset 0, ip.cc:87) of TCP (tcp.hh:852-862, 20 B
//    header) or UDP (udp.cc:153-161, 8 B) the port bytes at +20
//    (sizeof(ip_hdr): options are not skipped), if the frame holds them.
//  REASSEMBLED (ip.cc:186-197): src, dst; then the ports at 4*ihl when the
//    L4 part, up to min(ip_len, len), holds the TCP / UDP header.
// Returns false (hash 0) for a malformed frame: shorter than 20 B, or (mode 1)
// 4*ihl past the end of the datagram.
__device__ __forceinline__ bool rss_ipv4(const RssParams& P, uint32_t h0, uint32_t h1, uint32_t h2, uint32_t h3,
                                         uint32_t h4, uint32_t ports20, uint32_t ports_l4, uint32_t L,
                                         uint32_t& hash) {
    const uint32_t proto = (h2 >> 8) & 0xffu;
    const uint32_t need = proto == 6u ? 20u : (proto == 17u ? 8u : 0u);
    uint32_t ports = 0;
    if (P.mode == SCCSUM_RSS_DISPATCH) {
        const uint32_t frag = swap16(h1 >> 16);  // flags + fragment offset (ip.hh:390-391)
        if (need && (frag & 0x3fffu) == 0u && L >= 20u + need) ports = ports20;
    } else {
        const uint32_t l4_off = 4u * (h0 & 0xfu);
        const uint32_t ip_len = swap16(h0 >> 16);
        const uint32_t l4_end = ip_len < L ? ip_len : L;
        if (l4_off > l4_end) {
            hash = 0;
            return false;
        }
        if (need && l4_end - l4_off >= need) ports = ports_l4;
    }
    hash = toeplitz96(P, bswap32(h3), bswap32(h4), bswap32(ports));
    return true;
}

// Standalone RSS over a frame batch: one thread per frame, header dwords
// loaded aligned and re-aligned with v_alignbyte (frames at any offset; the
// buffer is readable to round16(bytes_len)).
__global__ __launch_bounds__(kBlock) void rss_kernel(const uint8_t* __restrict__ bytes, uint64_t bytes_len,
                                                     const uint64_t* __restrict__ off,
                                                     const uint32_t* __restrict__ len, uint8_t* __restrict__ status,
                                                     uint64_t n, const RssParams P) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = off[i];
    const uint32_t L = len[i];
    uint32_t hash = 0, st = 0;
    if (o > bytes_len || L > bytes_len - o) {
        st = SCCSUM_ST_RANGE;
    } else if (L < 20u) {
        st = SCCSUM_ST_MALFORMED;
    } else {
        const uint8_t* p = bytes + o;
        const uint32_t sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p) & 3u);
        const uint64_t padded = (bytes_len + 15u) & ~uint64_t(15);  // readable extent of the buffer
        auto dword_at = [&](uint64_t byte_off) -> uint32_t {          // aligned dword at bytes + byte_off
            return byte_off + 4u <= padded ? *reinterpret_cast<const uint32_t*>(bytes + byte_off) : 0u;
        };
        uint32_t d[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) d[k] = dword_at(o - sh + 4u * k);  // bytes [-sh, 28 - sh) of the frame
        const uint32_t h0 = __builtin_amdgcn_alignbyte(d[1], d[0], sh), h1 = __builtin_amdgcn_alignbyte(d[2], d[1], sh);
        const uint32_t h2 = __builtin_amdgcn_alignbyte(d[3], d[2], sh), h3 = __builtin_amdgcn_alignbyte(d[4], d[3], sh);
        const uint32_t h4 = __builtin_amdgcn_alignbyte(d[5], d[4], sh), h5 = __builtin_amdgcn_alignbyte(d[6], d[5], sh);
        uint32_t pl = h5;
        const uint32_t l4_off = 4u * (h0 & 0xfu);
        if (P.mode != SCCSUM_RSS_DISPATCH && l4_off != 20u && l4_off + 4u <= L) {
            const uint64_t q = o + l4_off - sh;
            pl = __builtin_amdgcn_alignbyte(dword_at(q + 4u), dword_at(q), sh);
        }
        if (!rss_ipv4(P, h0, h1, h2, h3, h4, h5, pl, L, hash)) st = SCCSUM_ST_MALFORMED;
    }
    P.hash[i] = hash;
    if (status) status[i] = static_cast<uint8_t>(st);
}

// ---------------------------------------------------------------- flat kernel

// Inclusive prefix sums over the 64 lanes: Hillis-Steele row scans by
// row_shr 1/2/4/8 (zero fill at the row edge), then row_bcast 15/31 carry the
// row totals into rows 1-3 (gfx9 DPP; six v_add_u32_dpp per value).
// tools/dev/scan_check.hip checks the sequence lane by lane on the device.
// U independent scans, step-interleaved so that no DPP op
// reads the result of the instruction just before it (no hazard nops).
template <int U>
__device__ __forceinline__ void wave_scan_n(uint32_t (&x)[U]) {
#define SCCSUM_SCAN_STEP(ctrl, rm, bm)                                                                          \
    _Pragma("unroll") for (int u = 0; u < U; ++u) x[u] +=                                                       \
        static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x[u]), ctrl, rm, bm, true));
    SCCSUM_SCAN_STEP(0x111, 0xF, 0xF)
    SCCSUM_SCAN_STEP(0x112, 0xF, 0xF)
    SCCSUM_SCAN_STEP(0x114, 0xF, 0xF)
    SCCSUM_SCAN_STEP(0x118, 0xF, 0xF)
    SCCSUM_SCAN_STEP(0x142, 0xA, 0xF)
    SCCSUM_SCAN_STEP(0x143, 0xC, 0xF)
#undef SCCSUM_SCAN_STEP
}

// Dword i of the 64 bytes held in four units.
__device__ __forceinline__ uint32_t unit_dword(const u32x4 (&h)[4], int i) {
    const u32x4& u = h[i >> 2];
    return (i & 3) == 0 ? u.x : (i & 3) == 1 ? u.y : (i & 3) == 2 ? u.z : u.w;
}

// The dword at byte `head + 4 i` of the four units (head < 16): a 4-way
// select on head / 4 and a byte funnel shift.
__device__ __forceinline__ uint32_t header_dword(const u32x4 (&h)[4], uint32_t head, int i) {
    const uint32_t q = head >> 2;
    auto pick = [&](int j) {
        const uint32_t a = unit_dword(h, j), b = unit_dword(h, j + 1), c = unit_dword(h, j + 2),
                       d = unit_dword(h, j + 3);
        return q == 0 ? a : q == 1 ? b : q == 2 ? c : d;
    };
    return __builtin_amdgcn_alignbyte(pick(i + 1), pick(i), head & 3u);
}

// Output stores of a tile (diagnostic A/B of the cache policy, flags bits
// kOutPolicyShift..+2): 0 = plain global store; buffer stores with 1 = nt,
// 2 = sc1, 3 = sc0 sc1, 4 = sc0.  t + lane is the element this lane writes.
constexpr uint32_t kOutPolicyShift = 8;
template <typename T>
__device__ __forceinline__ void tile_store(T* t, uint32_t lane, T v, uint32_t pol) {
    if (pol == 0) {
        gst(t)[lane] = v;
        return;
    }
    const auto r = rsrc(reinterpret_cast<const uint8_t*>(t), 64u * sizeof(T));
    const int o = static_cast<int>(sizeof(T) * lane);
    auto st = [&](auto aux) {
        constexpr int a = decltype(aux)::value;
        if constexpr (sizeof(T) == 4) {
            __builtin_amdgcn_raw_buffer_store_b32(static_cast<uint32_t>(v), r, o, 0, a);
        } else if constexpr (sizeof(T) == 2) {
            __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(v), r, o, 0, a);
        } else {
            __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(v), r, o, 0, a);
        }
    };
    switch (pol) {
        case 1: st(std::integral_constant<int, 2>{}); break;
        case 2: st(std::integral_constant<int, 16>{}); break;
        case 3: st(std::integral_constant<int, 17>{}); break;
        default: st(std::integral_constant<int, 1>{}); break;
    }
}

// Sparse layouts (variant 2): a wave owns TILES of 64 consecutive packets, as
// the flat kernel does, but loads them ROW by row — one packet per 16-lane
// row, four packets per load instruction, V 16-byte units per lane — because
// in a sparse layout (DPDK mbuf slots a NIC wrote into HBM: 1500 B of every
// 2304) every packet is its own run and the flat kernel's wave would wait
// out one memory round trip per packet.  The rows do only what the bytes
// need: load, v_sad_u16 the whole units, a row sum (DPP), and hand the
// packet's lane its sum plus the units its finish needs (the first three,
// the last) through LDS.  Everything per packet — IPv4 header, the edge
// bytes outside the summed range, pseudo-header, fold, result — then runs
// lane-parallel once per tile for all 64 packets (the flat kernel's phase C),
// instead of once per row step for four: round 2's row kernel spent ~350
// vector instructions per four packets on it and ran at 74 % where its own
// loads alone reach 81 % (profiles/r03_sparse_probe.log).  Frames the fast
// path cannot take (IP options, a trimmed IP length, over 128 KiB) are redone
// exactly, one wave each (the flat kernel's phase D); results leave as one
// coalesced store per tile.
// One checksum field of an in-place fill (2 bytes, little-endian as the
// kernels hold it; byte stores at odd addresses).  kWriteThrough: sc0 sc1.
template <bool kWriteThrough>
__device__ __forceinline__ void store_field(uint8_t* p, uint32_t v) {
    if ((reinterpret_cast<uintptr_t>(p) & 1u) == 0u) {
        if constexpr (kWriteThrough) {
            __hip_atomic_store(gst(reinterpret_cast<uint16_t*>(p)), static_cast<uint16_t>(v), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
#ifdef SCCSUM_AB_FILLSTORE_NT
            __builtin_nontemporal_store(static_cast<uint16_t>(v), reinterpret_cast<uint16_t*>(p));
#else
            *gst(reinterpret_cast<uint16_t*>(p)) = static_cast<uint16_t>(v);
#endif
        }
    } else if constexpr (kWriteThrough) {
        __hip_atomic_store(gst(p), static_cast<uint8_t>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(gst(p + 1), static_cast<uint8_t>(v >> 8), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
        gst(p)[0] = static_cast<uint8_t>(v);
        gst(p)[1] = static_cast<uint8_t>(v >> 8);
    }
}

// Several batches in one row-kernel launch (MQ: small sccsum_*_multi
// launches, whose batches would otherwise wait on the flat kernel's longer
// plan): packet p of the launch is packet p - first[q] of batch q.
constexpr uint32_t kRowQueues = 16;
struct RowQueues {
    uint32_t nq;
    uint64_t first[kRowQueues + 1];
    const uint8_t* bytes[kRowQueues];
    uint64_t bytes_len[kRowQueues];
    const uint64_t* off[kRowQueues];
    const uint32_t* len[kRowQueues];
    const uint32_t* seed[kRowQueues];
    uint16_t* out[kRowQueues];
    uint8_t* status[kRowQueues];
};
// a[q] for a lane-varying q with constant indices only (no private-memory copy of the argument)
template <class T>
__device__ __forceinline__ T row_pick(const T (&a)[kRowQueues], uint32_t q) {
    T r = a[0];
#pragma unroll
    for (uint32_t i = 1; i < kRowQueues; ++i) r = q == i ? a[i] : r;
    return r;
}

template <int V, bool IPV4, bool MQ = false, bool FILL = false>
__global__ __launch_bounds__(kBlock) void csum_row_kernel(
    const uint8_t* __restrict__ bytes, uint64_t bytes_len,
    const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
    const uint32_t* __restrict__ seed, uint16_t* __restrict__ out,
    uint8_t* __restrict__ status, uint64_t n, uint32_t flags, const RowQueues rq) {
    static_assert(!FILL || IPV4, "in-place fill is a frames mode");
    constexpr uint32_t kRow = 16;
    const bool raw = !IPV4 && (flags & kFlagRaw);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t r = lane & (kRow - 1), j = lane / kRow;  // lane r of row j
    // per packet of the tile: units 0, 1, 2 (3 too for a fill: the TCP field
    // may lie in it) and its last unit, for its finish
    constexpr int kPick = FILL ? 5 : 4;
    __shared__ u32x4 picks_all[kWavesPerBlock][kWave][kPick];
    u32x4(*picks)[kPick] = picks_all[wv];
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
    const uint64_t wglob = static_cast<uint64_t>(xcd_block_id()) * kWavesPerBlock + wv;
    // 64-packet tiles dealt round robin for as many whole rounds of the grid
    // as the batch holds (all waves sweep the buffer together, front to
    // back), then the packets left are split evenly over the waves as one
    // last short tile each, in wave order: 1 M packets over 6 144 resident
    // waves were 2.67 rounds, whose last third ran on 2/3 of the waves.
    // (Giving each wave one contiguous n / W share instead lost 1.5 %: 6 144
    // streams over the whole buffer; profiles/r03_ab_rows_partition.log.)
    const uint64_t R = (n / kWave) / nwaves;  // whole rounds of whole tiles
    const uint64_t rest0 = R * nwaves * kWave, rn = n - rest0;
    const uint64_t per = rn / nwaves, extra = rn % nwaves;  // per + 1 <= 64
    const uint64_t lo_last = rest0 + per * wglob + (wglob < extra ? wglob : extra);
    const uint32_t cnt_last = static_cast<uint32_t>(per + (wglob < extra ? 1u : 0u));
    for (uint64_t rr = 0; rr <= R; ++rr) {
        const uint64_t t0 = rr < R ? (rr * nwaves + wglob) * kWave : lo_last;
        const uint32_t cnt = rr < R ? static_cast<uint32_t>(kWave) : cnt_last;
        if (cnt == 0) break;
        // ---- A: lane k plans packet k of the tile (coalesced metadata loads)
        const uint64_t p = t0 + lane;
        const bool mine = lane < cnt;
        // the packet's batch: the kernel's one, or (MQ) the one p falls in
        const uint8_t* qbytes = bytes;
        uint64_t qbytes_len = bytes_len, lp = p;
        const uint64_t* qoff = off;
        const uint32_t *qlen = len, *qseed = seed;
        uint16_t* qout = out;
        uint8_t* qstatus = status;
        if constexpr (MQ) {
            uint32_t q = 0;
#pragma unroll
            for (uint32_t i = 1; i < kRowQueues; ++i) q += (i < rq.nq && p >= rq.first[i]) ? 1u : 0u;
            lp = p - row_pick(*reinterpret_cast<const uint64_t(*)[kRowQueues]>(rq.first), q);
            qbytes = row_pick(rq.bytes, q);
            qbytes_len = row_pick(rq.bytes_len, q);
            qoff = row_pick(rq.off, q);
            qlen = row_pick(rq.len, q);
            qseed = row_pick(rq.seed, q);
            qout = row_pick(rq.out, q);
            qstatus = row_pick(rq.status, q);
        }
        const uint64_t o = mine ? qoff[lp] : 0;
        const uint32_t L = mine ? qlen[lp] : 0u;
        const uint32_t sd = (!IPV4 && qseed && mine) ? qseed[lp] : 0u;
        const bool range_bad = mine && (o > qbytes_len || L > qbytes_len - o);
        const bool short_frame = IPV4 && mine && !range_bad && L < 20;
        const bool huge = mine && !range_bad && L > kExactMax;
        const bool fast = mine && !range_bad && !short_frame && !huge;
        const uint64_t ptr = reinterpret_cast<uint64_t>(qbytes) + (range_bad ? 0 : o);
        const uint32_t head = static_cast<uint32_t>(ptr & 15u);
        const uint64_t a0 = ptr - head;
        const uint32_t nunits = (fast && L) ? (head + L + 15u) >> 4 : 0u;

        // ---- B: rows load and sum; packet k's sum and picks go to lane k
        uint32_t res = 0;
        for (uint32_t s = 0; s * 4u < cnt; ++s) {
            const uint32_t k = 4u * s + j;  // this row's packet
            const uint32_t klo = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(a0)), k));
            const uint32_t khi = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(a0 >> 32)), k));
            const uint32_t knu = static_cast<uint32_t>(__shfl(static_cast<int>(nunits), k));
            const uint8_t* lb = reinterpret_cast<const uint8_t*>((static_cast<uint64_t>(khi) << 32) | klo) + 16u * r;
            uint32_t sum = 0;
            for (uint32_t g = 0; g < knu; g += V * kRow) {
                const int lim = static_cast<int>(knu) - static_cast<int>(g + r);  // this lane's units left
                u32x4 v[V];
#pragma unroll
                for (int u = 0; u < V; ++u) {
                    v[u] = u * static_cast<int>(kRow) < lim ? load_unit(lb + 16u * g + 256u * u) : u32x4{0, 0, 0, 0};
                }
#pragma unroll
                for (int u = 0; u < V; ++u) sum = sad4(v[u], sum);
                if (g == 0 && r < static_cast<uint32_t>(kPick - 1)) picks[k][r] = v[0];  // units 0..2 (3) (zero past the packet)
                // the lane holding the last unit (its unit u has lim - 1 == 16 u): select, then one store
                u32x4 lastv = v[0];
#pragma unroll
                for (int u = 1; u < V; ++u) lastv = lim - 1 == 16 * u ? v[u] : lastv;
                if (lim >= 1 && lim <= 16 * V && ((lim - 1) & 15) == 0) picks[k][kPick - 1] = lastv;
            }
            // row sums (exact: < 2^32 up to kExactMax bytes), one per row, to the packets' lanes
            const uint32_t rsum = row_sum(sum);
#pragma unroll
            for (uint32_t jj = 0; jj < 4; ++jj) {
                const uint32_t sj = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(rsum), 16 * jj));
                res = lane == 4u * s + jj ? sj : res;
            }
        }
        __builtin_amdgcn_wave_barrier();  // the rows' LDS picks precede the lanes' reads

        // ---- C: lane k finishes packet k
        u32x4 hs[4] = {picks[lane][0], picks[lane][1], picks[lane][2], FILL ? picks[lane][3] : u32x4{0, 0, 0, 0}};
        const u32x4 hl = picks[lane][kPick - 1];
        __builtin_amdgcn_wave_barrier();  // this tile's reads precede the next tile's writes
        if (FILL && huge) {
            // a frame over 128 KiB was not streamed (no row loaded it, so its
            // picks hold another tile's bytes): its header straight from the
            // frame — 64 bytes from a0, inside it — for the decisions below,
            // and phase D sums it exactly (max_len is only a hint: ADVICE r05)
#pragma unroll
            for (int u = 0; u < 4; ++u) hs[u] = load_unit(reinterpret_cast<const uint8_t*>(a0) + 16u * u);
        }
        // a fill's ICMP echo request: the reply's sum skips type, code and checksum (as flat_body)
        const bool icmp_lane = FILL && (flags & kFlagFillIcmp) && mine && !range_bad && !short_frame &&
                               ((header_dword(hs, head, 2) >> 8) & 0xffu) == 1u;
        const int rs0 = static_cast<int>(head) + (IPV4 ? 20 + (icmp_lane ? 4 : 0) : 0);
        const int re0 = static_cast<int>(head + L);
        const int lastu16 = 16 * (static_cast<int>(nunits) - 1);
        uint32_t excl = unit_part(hs[0], 0, rs0);
        if (IPV4) excl += unit_part(hs[1], 0, rs0 - 16) + unit_part(hs[2], 0, rs0 - 32);
        excl += unit_part(hl, re0 - lastu16, 16);
        const uint32_t kept = nunits ? res - excl : 0u;
        uint32_t S = fold16(kept);
        if (head & 1u) S = swap16(S);
        uint32_t word = 0, st = 0, ipc = 0, pseudo = 0, fpos = 0, srs = 0, sre = 0;
        bool slow = huge;  // (not streamed: phase D decodes its header from the frame)
        if (FILL) {
            // in-place generate, one pass: flat_body's fill finish (phase C), then
            // the stores below (a huge frame's L4 sum is phase D's exact redo)
            const uint32_t h0 = header_dword(hs, head, 0), h1 = header_dword(hs, head, 1);
            const uint32_t h2 = header_dword(hs, head, 2), h3 = header_dword(hs, head, 3);
            const uint32_t h4 = header_dword(hs, head, 4);
            const FrameDecode D = frame_decode(h0, h1, h2, h3, h4, L);
            ipc = ~fold16(static_cast<uint64_t>(h0) + h1 + (h2 & 0xffffu) + h3 + h4) & 0xffffu;
            st = D.st;
            pseudo = D.pseudo;
            const bool need = fast && (D.ihl != 5u || D.ip_len != L);
            const bool atomic = (st & (SCCSUM_ST_MALFORMED | SCCSUM_ST_IPFRAG)) == 0u && D.ihl >= 5u;
            uint32_t fo = 0;
            if ((flags & kFlagFillL4) && (D.proto == 17u || D.proto == 6u)) fo = D.proto == 17u ? 6u : 16u;
            if (icmp_lane && atomic && D.l4_len >= 8u) {
                const uint32_t type = D.ihl == 5u ? header_dword(hs, head, 5) & 0xffu
                                                  : reinterpret_cast<const uint8_t*>(a0)[head + D.l4_off];
                fo = type == 8u ? 2u : 0u;
            }
            const bool has_field = fo != 0u && atomic && D.l4_len >= fo + 2u;
            fpos = has_field ? head + D.l4_off + fo : 0u;
            srs = head + D.l4_off + (icmp_lane ? 4u : 0u);
            sre = head + D.l4_off + D.l4_len;
            uint32_t rr;
            if (icmp_lane) {
                rr = ~S & 0xffffu;
            } else {
                uint32_t fv = 0;
                if (has_field && !need) fv = fo == 6u ? header_dword(hs, head, 6) >> 16 : header_dword(hs, head, 9) & 0xffffu;
                rr = ~fold16(static_cast<uint64_t>(S) + pseudo + (~fv & 0xffffu)) & 0xffffu;
            }
            const bool fill_ip = (flags & kFlagFillIp) != 0u;
            word = (fill_ip ? ipc : 0u) | (has_field ? rr << 16 : 0u);
            st |= (fill_ip ? SCCSUM_ST_OK : 0u) | (has_field ? SCCSUM_ST_L4_OK : 0u);
            slow = (need || huge) && has_field;
        } else if (IPV4) {
            const uint32_t h0 = header_dword(hs, head, 0), h1 = header_dword(hs, head, 1);
            const uint32_t h2 = header_dword(hs, head, 2), h3 = header_dword(hs, head, 3);
            const uint32_t h4 = header_dword(hs, head, 4);
            const FrameDecode D = frame_decode(h0, h1, h2, h3, h4, L);
            ipc = ~fold16(static_cast<uint64_t>(h0) + h1 + h2 + h3 + h4) & 0xffffu;
            st = D.st;
            pseudo = D.pseudo;
            // options or a trimmed IP length: the exact redo (a fragment claims no L4 value)
            if (fast && (D.ihl != 5u || D.ip_len != L) && (st & SCCSUM_ST_IPFRAG) == 0u) slow = true;
            const uint32_t rr = ~fold16(static_cast<uint64_t>(S) + pseudo) & 0xffffu;
            word = frame_word(ipc, rr, st);
            st = frame_status(ipc, rr, st);
        } else {
            const uint32_t rr = raw ? S : ~fold16(static_cast<uint64_t>(S) + swap16(fold16(sd))) & 0xffffu;
            word = rr;
            st = (!raw && rr == 0) ? SCCSUM_ST_OK : 0u;
        }
        if (range_bad) {
            word = 0;
            st = SCCSUM_ST_RANGE;
        } else if (short_frame) {
            word = 0;
            st = SCCSUM_ST_MALFORMED;
        }

        // ---- D: exact redo of the packets the fast path could not take (frame
        // header from the packet itself when it was not streamed: over 128 KiB)
        uint64_t todo = __ballot(slow);
        while (todo) {
            const uint32_t jl = static_cast<uint32_t>(__builtin_ctzll(todo));
            todo &= todo - 1;
            const uint32_t jlo = __builtin_amdgcn_readlane(static_cast<uint32_t>(a0), jl);
            const uint32_t jhi = __builtin_amdgcn_readlane(static_cast<uint32_t>(a0 >> 32), jl);
            const uint8_t* ja0 = reinterpret_cast<const uint8_t*>((static_cast<uint64_t>(jhi) << 32) | jlo);
            const uint32_t jhead = __builtin_amdgcn_readlane(head, jl);
            const uint32_t jL = __builtin_amdgcn_readlane(L, jl);
            uint64_t rs = jhead, re = static_cast<uint64_t>(jhead) + jL;
            uint32_t jipc = 0, jpseudo = 0, jst = 0;
            if (FILL) {  // the lane's own decisions from phase C (options or a trimmed IP length)
                rs = static_cast<uint32_t>(__builtin_amdgcn_readlane(srs, jl));
                re = static_cast<uint32_t>(__builtin_amdgcn_readlane(sre, jl));
            } else if (IPV4) {
                // the header from the frame itself (wave-uniform; over 128 KiB it was not picked
                // up).  Dword 5 only when the header is not dword-aligned: for an aligned 20-byte
                // frame it would lie past the frame, possibly past roundup(bytes_len, 16)
                // (global address space: a FLAT load would count against both wait
                // counters and make the compiler's later waits conservative)
                const auto* hp = gld(reinterpret_cast<const uint32_t*>(ja0 + jhead - (jhead & 3u)));
                const uint32_t sh = jhead & 3u;
                uint32_t hd[6];
#pragma unroll
                for (int i = 0; i < 5; ++i) hd[i] = hp[i];
                hd[5] = sh ? hp[5] : 0u;
                uint32_t h[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) h[i] = __builtin_amdgcn_alignbyte(hd[i + 1], hd[i], sh);
                const FrameDecode D = frame_decode(h[0], h[1], h[2], h[3], h[4], jL);
                jipc = ~fold16(static_cast<uint64_t>(h[0]) + h[1] + h[2] + h[3] + h[4]) & 0xffffu;
                jpseudo = D.pseudo;
                jst = D.st;
                rs = jhead + D.l4_off;
                re = rs + D.l4_len;
            }
            uint32_t SJ = exact_range_sum(ja0, rs, re, lane);
            if (jhead & 1u) SJ = swap16(SJ);
            if (lane == jl) {
                if (FILL) {
                    uint32_t rr = ~SJ & 0xffffu;  // ICMP echo: the message after type, code, checksum
                    if (!icmp_lane) {
                        const uint8_t* fp = reinterpret_cast<const uint8_t*>(a0) + fpos;
                        const uint32_t fv = static_cast<uint32_t>(fp[0]) | (static_cast<uint32_t>(fp[1]) << 8);
                        rr = ~fold16(static_cast<uint64_t>(SJ) + pseudo + (~fv & 0xffffu)) & 0xffffu;
                    }
                    word = (word & 0xffffu) | (rr << 16);
                } else if (IPV4) {
                    const uint32_t rr = ~fold16(static_cast<uint64_t>(SJ) + jpseudo) & 0xffffu;
                    word = frame_word(jipc, rr, jst);
                    st = frame_status(jipc, rr, jst);
                } else {
                    const uint32_t rr = raw ? SJ : ~fold16(static_cast<uint64_t>(SJ) + swap16(fold16(sd))) & 0xffffu;
                    word = rr;
                    st = (!raw && rr == 0) ? SCCSUM_ST_OK : 0u;
                }
            }
        }
        if (FILL && mine) {  // the fields, after every read of the tile (st: which were generated)
            uint8_t* const f0 = reinterpret_cast<uint8_t*>(a0);
            if (st & SCCSUM_ST_OK) store_field<false>(f0 + head + 10, word);
            if (st & SCCSUM_ST_L4_OK) {
                if (icmp_lane) store_field<false>(f0 + fpos - 2, 0u);  // echo reply: type 0, code 0
                store_field<false>(f0 + fpos, word >> 16);
            }
        }
        if (mine) {
            if (IPV4) {
                if (qout) reinterpret_cast<uint32_t*>(qout)[lp] = word;
            } else {
                qout[lp] = static_cast<uint16_t>(word);
            }
            if (qstatus) qstatus[lp] = static_cast<uint8_t>(st);
        }
    }
}

#ifdef SCCSUM_AB_TIMELINE
// A/B diagnostic only (tools/build_ab.sh timeline=SCCSUM_AB_TIMELINE,
// tools/dev/timeline_probe.py): per wave of the last flat launch, the
// constant-clock times (100 MHz) of its start, its first chunk's data in
// registers, its failing dequeue, and its tile count.
constexpr uint32_t kTimelineWaves = 16384;
__device__ unsigned long long g_timeline[kTimelineWaves][4];
// engine runs: per wave, [waits that slept, ticks asleep, mirror reloads,
// descriptor walks, ticks in walks, flushes, ticks in flushes, host polls]
__device__ unsigned long long g_engine_stats[kTimelineWaves][8];
// engine runs, per step of the run (the first kStepRec): the latest tile
// retire of each dequeue group, and per XCD the latest and (complemented, so a
// max keeps the earliest) first tile retire
constexpr uint32_t kStepRec = 1024;
__device__ unsigned long long g_step_grp[kStepRec][64];
__device__ unsigned long long g_step_xcd[kStepRec][8][2];
#endif

constexpr int kGapUnits = 4;  // flat runs tolerate gaps of up to 4 units (64 B) between packets


// The batches one flat-kernel launch works through: up to kMaxQueues
// independent batches (rx / tx queues, the tx and rx halves of a step), each
// with its own bytes, offsets, lengths, seeds and outputs.  Tiles are numbered
// across the batches (tile0 = prefix of their tile counts), so one grid, one
// ramp and one drain serve them all.  Passed by value (kernel arguments).
constexpr uint32_t kMaxQueues = 16;
struct Queues {
    uint32_t nq;
    // Tail split: tiles from `tsplit` on (the launch's last ones, dequeued
    // last) are cut into 2^sub_log2 sub-tiles of `bsub` packets, so the
    // launch's drain waits on short tiles.  Tile numbers are virtual:
    // [0, tsplit) are whole tiles, then sub-tile s of whole tile
    // tsplit + (v - tsplit) >> sub_log2.
    uint64_t tsplit;
    uint32_t sub_log2, bsub;
    uint64_t tile0[kMaxQueues + 1];
    const uint8_t* bytes[kMaxQueues];
    uint64_t bytes_len[kMaxQueues];
    const uint64_t* off[kMaxQueues];
    const uint32_t* len[kMaxQueues];
    const uint32_t* seed[kMaxQueues];
    uint16_t* out[kMaxQueues];
    uint8_t* status[kMaxQueues];
    uint64_t n[kMaxQueues];
};

// Flat kernel.  Wave w owns tiles of B <= 64 consecutive packets (one per
// lane); the bytes are streamed per RUN, not per packet: a run is a maximal
// sequence of tile packets whose 16-byte unit spans go forward with gaps of
// at most kGapUnits (packed batches: the whole tile).  The wave reads the
// run's unit extent densely — U units per lane per chunk, no empty lane
// loads whatever the packet sizes — sums each unit (v_sad_u16), takes a
// wave-wide inclusive prefix scan of the unit sums (DPP) and parks the chunk's
// prefix values and units in LDS; every packet lane then picks up the prefix
// just before its first unit and at its last unit, plus the units the
// finishing step needs (the first 1/3/4 units, the last), when they pass.  A
// packet's sum of units is the difference of its two prefix values (exact
// mod 2^32; sums stay below 2^32 up to kExactMax bytes), after which the
// finishing step (edge bytes, IPv4 header, pseudo-header) runs lane-parallel
// and the packets the fast path cannot take are redone exactly, one wave each.
// Layouts that do not run forward (shuffled offsets) degrade to one run per
// packet.
// (waves_per_eu: the U = 8 forms fit 168 VGPRs and keep 3 waves per SIMD —
// the in-place form with a chunk in flight needed 172 without the bound; the
// U = 16 forms are held to 2 by their LDS anyway)
// A flat launch's tiles come from a tile SOURCE: QueueSrc (one launch over
// the queue set in its arguments, csum_flat_kernel) or EngineSrc (a resident
// grid fed steps through a ring, csum_engine_kernel, §5.11 of DESIGN.md).
// Both give the same body (flat_body) a tile's batch and packet range (Ref),
// the next tile number to work on, and what to do once a tile is stored.
// A wave's dequeue group.  Each aligned run of 64 waves holds one wave of
// every group (a launch's per-group dequeue counts rely on it), shifted by one
// per run, so group g holds waves of every slot in their workgroup on every
// XCD; g = wglob % 64 gave a group waves of one slot only.  Waves are not
// equally fast and a group's are fixed, so in a long engine run the groups
// drift apart (the grid then works on several steps at once, its step time
// rising with the spread); this composition halves the drift rate
// (profiles/r04_engine_groups.log).
__device__ __forceinline__ uint32_t group_of(uint64_t wglob) {
    return static_cast<uint32_t>((wglob + wglob / kGroups) % kGroups);
}

struct QueueSrc {
    static constexpr bool kEngine = false;
    const Queues& Q;
    const uint32_t B;
    uint32_t* const heads;
    uint32_t* const done;
    const uint32_t ticket;
    uint64_t ntiles = 0, nwaves = 0, wglob = 0;
    uint32_t grp = 0, tiles_g = 0, waves_g = 0, lane = 0;
    struct Ref {
        uint32_t q, cnt;
        uint64_t base;
    };
    __device__ QueueSrc(const Queues& q, uint32_t b, uint32_t* h, uint32_t* d, uint32_t tk)
        : Q(q), B(b), heads(h), done(d), ticket(tk) {}
    __device__ void init(uint64_t wglob_, uint64_t nwaves_, uint32_t lane_) {
        // B packets per whole tile, numbered across the queues; the tail's whole
        // tiles count 2^sub_log2 virtual tiles each
        ntiles = Q.tsplit + ((Q.tile0[Q.nq] - Q.tsplit) << Q.sub_log2);
        nwaves = nwaves_;
        wglob = wglob_;
        lane = lane_;
        grp = group_of(wglob);
        const uint64_t rest = ntiles > nwaves ? ntiles - nwaves : 0;
        tiles_g = rest > grp ? static_cast<uint32_t>((rest - grp + kGroups - 1) / kGroups) : 0u;
        waves_g = static_cast<uint32_t>(nwaves / kGroups);
    }
    __device__ uint64_t end() const { return ntiles; }
    // (wave-uniform) virtual tile tt -> its queue, first packet and packet
    // count (0 for a sub-tile past the end of a short last tile): a scalar
    // walk over <= kMaxQueues prefixes
    __device__ Ref ref(uint64_t tt) const {
        const bool sub = tt >= Q.tsplit;
        const uint64_t w = sub ? Q.tsplit + ((tt - Q.tsplit) >> Q.sub_log2) : tt;
        Ref r;
        r.q = 0;
        while (r.q + 1 < Q.nq && w >= Q.tile0[r.q + 1]) ++r.q;
        r.base = (w - Q.tile0[r.q]) * B;
        const uint64_t left = Q.n[r.q] - r.base;  // >= 1
        r.cnt = left < B ? static_cast<uint32_t>(left) : B;
        if (sub) {
            const uint32_t s0 = static_cast<uint32_t>((tt - Q.tsplit) & ((1u << Q.sub_log2) - 1u)) * Q.bsub;
            const uint32_t c = s0 < r.cnt ? r.cnt - s0 : 0u;
            r.base += s0 < r.cnt ? s0 : 0u;  // an empty sub-tile keeps a valid base
            r.cnt = c < Q.bsub ? c : Q.bsub;
        }
        return r;
    }
    __device__ const uint8_t* bytes(const Ref& r) const { return Q.bytes[r.q]; }
    __device__ uint64_t bytes_len(const Ref& r) const { return Q.bytes_len[r.q]; }
    __device__ const uint64_t* off(const Ref& r) const { return Q.off[r.q]; }
    __device__ const uint32_t* len(const Ref& r) const { return Q.len[r.q]; }
    __device__ const uint32_t* seed(const Ref& r) const { return Q.seed[r.q]; }
    __device__ uint16_t* out(const Ref& r) const { return Q.out[r.q]; }
    __device__ uint8_t* status(const Ref& r) const { return Q.status[r.q]; }
    __device__ uint32_t tile_packets(const Ref&) const { return B; }
    // a launch's tiles are all of one kind, its fill flags the kernel's
    __device__ bool is_store(const Ref&) const { return false; }
    __device__ uint32_t fill_flags(const Ref&, uint32_t flags) const { return flags; }
    __device__ uint32_t store_mode(const Ref&) const { return 0u; }

    // Tile order.  Wave w first takes tile w (static: no start-up contention).
    // With `heads`, the remaining tiles [W, ntiles) are split over kGroups
    // counters (each on its own line) and dequeued: wave w pulls
    // tile W + g + kGroups * atomicAdd(heads[g], 1) with g = group_of(w), so
    // waves that drew short tiles take more (Zipf batches).  Each group's
    // dequeue count is known — one per remaining tile of the group plus one
    // failing dequeue per wave of the group — so the wave that draws the last
    // number zeroes the counter for the slot's next launch (no memset), and
    // the last group to do so stores this launch's ticket to `done` (pinned
    // host memory): the host may then hand the slot to another launch
    // (acquire_heads).  Without `heads`: static round robin.
    // A claim in two halves, the atomic (claim_issue) and its read-back
    // (claim_resolve): the flat body issues a tile's claim after the previous
    // tile's last loads and reads it back after that tile; claim() does both
    // at once (a wave's first claims).
    struct Claim {
        uint32_t raw;
        uint64_t prev;
    };
    __device__ Claim claim_issue(uint64_t prev) {
        Claim c{0u, prev};
        if (heads != nullptr && lane == 0)
            c.raw = __hip_atomic_fetch_add(heads + grp * kHeadStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return c;
    }
    __device__ uint64_t claim_resolve(const Claim& c) {
        if (heads == nullptr) return c.prev + nwaves;
        uint32_t d = c.raw;
        if (lane == 0 && d == tiles_g + waves_g - 1) {
            uint32_t* h = heads + grp * kHeadStride;
            // The slot's words are only ever touched by agent-scope atomics,
            // which are performed at the device's coherence point; waiting
            // for each to complete (s_waitcnt) orders reset -> count ->
            // report without the L2 write-backs a release fence costs
            // (profiles/r03_ab_pool_rows.log).
            __hip_atomic_store(h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            uint32_t* const groups_done = heads + kGroups * kHeadStride;
            const uint32_t gd = __hip_atomic_fetch_add(groups_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (gd == kGroups - 1) {  // every group has reset: the slot is free for another launch
                __hip_atomic_store(groups_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(done, ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        d = __builtin_amdgcn_readfirstlane(d);
        return d < tiles_g ? nwaves + grp + static_cast<uint64_t>(kGroups) * d : ntiles;
    }
    __device__ uint64_t claim(uint64_t prev) { return claim_resolve(claim_issue(prev)); }
    __device__ uint64_t first() {
        uint64_t t = wglob;
        if (t >= ntiles && heads != nullptr) t = claim(t);
        return t;
    }
    // every tile of the launch is known at launch: nothing to wait for
    __device__ bool ready(uint64_t) { return true; }
    __device__ bool wait_ready(uint64_t) { return true; }
    __device__ void retire(const Ref&) {}
};

// ---- the resident engine (sccsum_engine_*)
//
// One grid stays resident and takes STEPS — up to kEngineQueues batches each,
// the tx and rx halves of a step, a shard's rx queues — that the host
// publishes while it runs.  A step is a 512-byte descriptor (one 8-byte word
// per lane); its tiles continue the run's global tile numbering, so tile v of
// the run is claimed from group counter v % kGroups exactly as in a launch,
// and step boundaries cost nothing: no kernel boundary, no ramp, no drain
// between steps.  The host writes the descriptor into pinned memory and raises
// `published_steps` (ctl[0]).  Host memory is read by ONE wave at a time: the
// wave that finds no published tile for its claim takes the poll token, reads
// ctl[0] (and stop) over PCIe, copies the new descriptors into a device ring
// and raises a device mirror of the published tiles; every other wave reads
// only the mirror and the device ring.  (With every waiting wave polling the
// host itself, 2 048 waves' reads flooded PCIe: a 262 144-frame step took
// 22 ms instead of 0.13 ms, profiles/r04m.)  A wave that claims a tile past
// the mirror finishes the tile it holds first and only then waits (sleeping),
// so a wave never waits while it holds published work.  Each tile's results
// are written through (sc0 sc1) and counted per step and group; the last count
// of a step stores the step's ticket into its pinned done word.  Exit: the
// host sets stop (ctl[8]); a wave that needs a tile past every published step
// then leaves — and so does one that finds the grid given no step for
// `idle_ticks` (the poller stamps the time it last saw a new step), raising
// ctl[16] first.
//
// In-place fill through the engine (sccsum_engine_submit_fill): a fill is two
// steps.  The GENERATE step runs the flat body's FILL phase C (values into the
// caller's out2, nothing stored in the frames); the STORE step that follows it
// has lane-per-frame tiles that store those values into the frames' fields.
// The store step depends on its generate step: a wave whose next tile lies in
// it waits (after finishing what it holds) until the generate step's count is
// complete, read from a device copy of the steps' done words.  No wave can
// wait on itself: a store tile is only ever waited on by a wave that holds
// nothing older, and every generate tile precedes it in its group's claim
// order, so the chain of waits runs to strictly older tiles and ends.
//
// Unbounded runs: the descriptors live in a RING of 2^k slots (step s in slot
// s & ring_mask), host and device alike, and so do the steps' done words.  The
// host publishes step s only once every step up to s - ring is done (a step
// without tiles is done once the poller has copied it), so a step that is not
// done always has its slot; a wave looking for the step of its claimed tile
// (not done: the wave holds it) finds it by probing slots (walk(): the next
// step, then galloping and binary search from its cursor), where a slot that
// holds another step means that step is done, and every step before it.  A
// probe decides from the step's seal, one 8-byte word (engine_seal.h), so the
// polling wave rewrites a reused slot in one phase: a torn read of the other
// words is never taken, as a wave reads a whole descriptor only for a step
// that is not done.
constexpr uint32_t kEngineSlotWords = 64;  // 512-byte descriptors
// completion counters: steps in flight at most.  Tiny steps are latency-bound
// (~45 us from publish to done), so their rate scales with the steps in
// flight: 5.1 / 2.9 / 1.5 / 0.89 us per 32-packet step at 8 / 16 / 32 / 64
// (profiles/r06_in_flight.log); 256 slots lift the old cap of 64.
constexpr uint32_t kEngineCountSlots = 256;
constexpr uint32_t kEngineMaxRing = 1u << 16;  // descriptor ring slots (2 x 32 MiB of descriptor rings at most)
constexpr uint32_t kEngineDefaultRing = 1024;
// descriptors the polling wave copies per round of its stores, their host
// reads in flight together (only a waiting wave polls, holding no tile: with
// the poll inside the tile loop, 4 or 8 pushed the fill engine kernel into
// 224 B of scratch).  16 against 8 at 128 steps in flight: 32 / 128 / 1 024-
// packet steps 0.63 / 1.03 / 3.02 against 0.70 / 1.10 / 3.10 us, the same
// registers (profiles/r06_in_flight.log).
#ifdef SCCSUM_AB_POLL_GROUP
constexpr uint32_t kPollGroup = SCCSUM_AB_POLL_GROUP;  // A/B only
#else
constexpr uint32_t kPollGroup = 16;
#endif
// the engine's per-tile checks: their slow paths placed out of the tile loop
#ifdef SCCSUM_AB_NO_EXPECT  // A/B only
#define SCCSUM_HOT(x) (x)
#else
#define SCCSUM_HOT(x) __builtin_expect(!!(x), 1)
#endif
// descriptor words
constexpr uint32_t kEdFirst = 0;   // the step's first tile in the run
constexpr uint32_t kEdTiles = 1;   // tiles | B (packets per tile) << 32
constexpr uint32_t kEdStep = 2;    // the step's seal (engine_seal: its index and where it ends, one word)
constexpr uint32_t kEdNq = 3;      // batches in the step (1..kEngineQueues)
constexpr uint32_t kEdTile0 = 4;   // tile0[0..nq]: the batches' first tiles within the step
constexpr uint32_t kEdQueue = 9;   // + 8 q: bytes, bytes_len, off, len, seed, out, status, n (q < 4: words 9-40)
constexpr uint32_t kEdKind = 41;   // kind | flat-body fill flags << 8 | public fill mode << 16
constexpr uint32_t kEdDep = 42;    // 0, or 1 + the step whose completion this step's tiles wait for
constexpr uint32_t kEdIndex = 43;  // the step's index in the run, whole
// The seal (kEdStep): engine_seal.h
// step kinds
constexpr uint32_t kStepSum = 0;        // checksums into out / status (sccsum_engine_submit)
constexpr uint32_t kStepFillGen = 1;    // fill, generate half: values into out2, status; frames untouched
constexpr uint32_t kStepFillStore = 2;  // fill, store half: out2's values into the frames' fields
constexpr uint32_t kStoreTilePackets = 256;  // store tiles: 4 frames per lane
constexpr uint32_t kEngineSyncEvery = 10;    // big steps: every 10th waits for the one before it
// Store tiles write each field through (sc0 sc1).  Stored plain (the L2
// merging a frame's two fields) with one system-scope release per wave at the
// step's flush instead, a fill step took 408 us against 328 (the releases'
// L2 write-backs, 2 048 per step, stall every wave; profiles/r05_engine_fill.log).
#if defined(SCCSUM_AB_FILLSTORE_PLAIN) || defined(SCCSUM_AB_FILLSTORE_NORELEASE)
constexpr bool kStoreWT = false;  // A/B only (NORELEASE: not even the release; results unsafe until the run ends)
#else
constexpr bool kStoreWT = true;
#endif
// ctl words (pinned): each on its own 64-byte line
constexpr uint32_t kEcPublished = 0, kEcStop = 8, kEcError = 16, kEcDone = 24;  // done[s] at 24 + 8 s
// kEcError values: the grid gave up waiting for a step (idle), or on a dependency, or a wave found no
// step holding its published tile (the last two are faults: never expected)
constexpr uint64_t kErrIdle = 1, kErrDepWait = 2, kErrWalk = 3;
// mirror words (device): published tiles, steps copied, stop seen, poll token, time of the last new step
constexpr uint32_t kMpTiles = 0, kMpSteps = 8, kMpStop = 16, kMpToken = 24, kMpStamp = 32, kMirrorWords = 40;

struct EngineArgs {
    const uint64_t* hring;  // descriptors as the host writes them, kEngineSlotWords words per slot (pinned)
    uint64_t* dring;        // the same descriptors, copied by the polling wave (device)
    uint64_t ring_mask;     // ring slots - 1 (a power of two): step s lives in slot s & ring_mask
    uint64_t* ctl;          // control words (device view of pinned memory)
    uint64_t* mirror;       // kMirrorWords (device)
    uint64_t* claims;       // kGroups 64-bit claim counters, 256 B apart (device; a run never wraps one)
    uint32_t* counts;       // kEngineCountSlots x kGroups completion counters, kHeadStride apart (device)
    uint32_t* gdone;        // kEngineCountSlots groups-done counters, kHeadStride apart (device)
    uint64_t* sdone;        // kEngineCountSlots words, 8 apart: 1 + the latest step done in each count slot (device)
    uint64_t idle_ticks;    // 100 MHz ticks the grid may go without a new step before a waiting wave gives up
    uint64_t dep_ticks;     // safety limit of a wait on a dependency (never reached by a correct run)
};

__device__ __forceinline__ uint64_t rfl64(uint64_t x) {
    return static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x)))) |
           static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32))))
               << 32;
}
__device__ __forceinline__ uint64_t rl64(uint64_t x, uint32_t k) {
    return static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(x), k))) |
           static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(x >> 32), k)))
               << 32;
}

// A fault ends the wave where it stands (reported first; the host sees
// SCCSUM_EFAULT).  (Returning it up through ready() / wait_ready() cost the
// kernel ~40 VGPRs of merged control flow in the tile loop.)
#ifdef SCCSUM_AB_NO_ENDPGM  // A/B only (a fault then runs on with a wrong cursor)
__device__ __forceinline__ void engine_fault(uint64_t* ctl, uint32_t lane, uint64_t code) {
    if (lane == 0) __hip_atomic_store(ctl + kEcError, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
#else
[[noreturn]] __device__ __forceinline__ void engine_fault(uint64_t* ctl, uint32_t lane, uint64_t code) {
    if (lane == 0) __hip_atomic_store(ctl + kEcError, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_endpgm();
}
#endif

struct WalkHit {
    uint64_t t, w;
};
// walk()'s search past the step after the cursor (below: a step before v's):
// galloping, bounded by the mirror's step count, then bisection for the first
// step whose seal does not lie before v, each probe one 8-byte read of a seal;
// then that step's whole descriptor, which no rewrite can touch (the step is
// not done: v is the caller's, unprocessed).  Out of line (a call, on a
// wave's rare long walk), and so are its faults: an s_endpgm anywhere in the
// kernel body's walk ran cfg 3 1.5-2 % slower on the same box, with or without
// the search inlined (profiles/r06_walk_ab.log).
__device__ __attribute__((noinline)) WalkHit engine_walk_far(const uint64_t* dring, uint64_t ring_mask,
                                                             const uint64_t* mirror, uint64_t* ctl, uint64_t below,
                                                             uint64_t v) {
    const uint32_t lane = __lane_id();
    uint64_t hs = 0;
    if (lane == 0) hs = __hip_atomic_load(mirror + kMpSteps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    hs = rfl64(hs);
    uint64_t above = hs;  // below lies before v's step; above does not (or is past every copied step)
    bool bisect = false;
    uint64_t d = 1;
    for (;;) {
        uint64_t t;
        if (!bisect) {
            t = below + d;
            if (t >= above) {
                bisect = true;
                continue;
            }
        } else {
            if (above <= below + 1) break;
            t = below + (above - below) / 2;
        }
        uint64_t p = 0;
        if (lane == 0) p = __hip_atomic_load(dring + (t & ring_mask) * kEngineSlotWords + kEdStep, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        p = rfl64(p);
        if (seal_before(p, t, v)) {
            below = t;
            d <<= 1;
        } else {
            above = t;
            bisect = true;
        }
    }
    if (above >= hs) engine_fault(ctl, lane, kErrWalk);  // a published tile in no published step
    const uint64_t w = __hip_atomic_load(dring + (above & ring_mask) * kEngineSlotWords + lane, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    if (rl64(w, kEdIndex) != above || v < rl64(w, kEdFirst) || seal_before(rl64(w, kEdStep), above, v)) {
        engine_fault(ctl, lane, kErrWalk);
    }
    return WalkHit{above, w};
}

struct EngineSrc {
    static constexpr bool kEngine = true;
    const EngineArgs& E;
    const bool wt;                                     // results written through (kFlagEngineWT)
    uint32_t lane = 0, grp = 0;
    uint64_t pub = 0;                                  // published tiles, as the mirror last said
    uint64_t step = ~0ull, sfirst = 0, slast = 0;      // the cursor: step `step` holds tiles [sfirst, slast)
    uint64_t dw = 0;                                   // lane i: word i of the cursor's descriptor
    uint64_t skind = 0, sdep = 0;                      // the cursor step's kind word and dependency
    uint64_t dep_seen = 0;                             // the latest dependency (1 + step) found done
#ifdef SCCSUM_AB_TIMELINE
    unsigned long long ab[8] = {};
#endif
    struct Ref {
        uint32_t cnt, B, kind;
        uint64_t base, step, first, last;
        const uint8_t* bytes;
        uint64_t bytes_len;
        const uint64_t* off;
        const uint32_t* len;
        const uint32_t* seed;
        uint16_t* out;
        uint8_t* status;
    };
    __device__ EngineSrc(const EngineArgs& e, uint32_t flags) : E(e), wt((flags & kFlagEngineWT) != 0) {}
    __device__ void init(uint64_t wglob, uint64_t, uint32_t lane_) {
        lane = lane_;
        grp = group_of(wglob);
    }
    __device__ uint64_t end() const { return ~0ull; }
    struct Claim {
        uint64_t raw;
    };
    __device__ Claim claim_issue(uint64_t) {
        Claim c{0u};
        if (lane == 0) c.raw = __hip_atomic_fetch_add(E.claims + grp * (kHeadStride / 2), 1ull, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
        return c;
    }
    __device__ uint64_t claim_resolve(const Claim& c) {
        const uint64_t d = rfl64(c.raw);
        return grp + static_cast<uint64_t>(kGroups) * d;
    }
    __device__ uint64_t claim(uint64_t prev) { return claim_resolve(claim_issue(prev)); }
    __device__ uint64_t ctl_load(uint32_t w) {  // host memory (PCIe): the poll token's holder only
        uint64_t v = 0;
        if (lane == 0) v = __hip_atomic_load(E.ctl + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return rfl64(v);
    }
    __device__ uint64_t mload(uint32_t w) {
        uint64_t v = 0;
        if (lane == 0) v = __hip_atomic_load(E.mirror + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return rfl64(v);
    }
    // Take the poll token if it is free; then bring the host's new steps into
    // the device ring and raise the mirror (tiles and steps, then stop: a
    // wave that sees stop then sees every step).
    __device__ void poll() {
        uint32_t got = 0;
        if (lane == 0 && __hip_atomic_load(E.mirror + kMpToken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
            uint64_t expect = 0;
            got = __hip_atomic_compare_exchange_strong(E.mirror + kMpToken, &expect, 1ull, __ATOMIC_RELAXED,
                                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                      ? 1u
                      : 0u;
        }
        if (!__builtin_amdgcn_readfirstlane(got)) return;
#ifdef SCCSUM_AB_TIMELINE
        ++ab[7];
#endif
        const uint64_t stop = ctl_load(kEcStop);  // before the steps: the host raises it after its last step
        const uint64_t hs = ctl_load(kEcPublished);
        uint64_t ms = mload(kMpSteps);
        const uint64_t ms0 = ms;
        uint64_t tiles = mload(kMpTiles);
        // Copy the new descriptors in groups: a group's host reads are in
        // flight together (one PCIe round trip), then its slots are rewritten
        // in one phase, reused or not: a probe of a slot it may be rewriting
        // reads only the seal (one 8-byte word, engine_seal), and a probe that
        // takes a whole descriptor does so only for a step that is not done,
        // whose slot the host has not handed on (round 6's first form wrote
        // reused slots in three waited phases: 0.1-0.25 us per tiny step,
        // profiles/r06_poller_phases_ab.log).
        auto dslot = [&](uint64_t s) { return E.dring + (s & E.ring_mask) * kEngineSlotWords + lane; };
        auto put = [&](uint64_t s, uint64_t x) {
            __hip_atomic_store(dslot(s), x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };
        while (ms < hs) {
            const uint64_t g = hs - ms < kPollGroup ? hs - ms : kPollGroup;
            uint64_t w[kPollGroup];
#pragma unroll
            for (uint32_t k = 0; k < kPollGroup; ++k) {
                w[k] = k < g ? __hip_atomic_load(E.hring + ((ms + k) & E.ring_mask) * kEngineSlotWords + lane,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                             : 0ull;
            }
#pragma unroll
            for (uint32_t k = 0; k < kPollGroup; ++k) {
                if (k < g) put(ms + k, w[k]);
            }
            // A step without tiles is done once copied: the poller says so.
            // (Marked done by the host at publication, it freed its host slot
            // before the poller had read it, and a run of such steps let the
            // host lap the ring past the copy: tests/test_gpu_engine.py
            // test_engine_walk_across_empty_steps.)
#pragma unroll
            for (uint32_t k = 0; k < kPollGroup; ++k) {
                if (k < g && static_cast<uint32_t>(rl64(w[k], kEdTiles)) == 0u && lane == 0) {
                    __hip_atomic_store(E.ctl + kEcDone + 8u * ((ms + k) & E.ring_mask), ms + k + 1, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < kPollGroup; ++k) {
                if (k + 1 == g) tiles = rl64(w[k], kEdFirst) + static_cast<uint32_t>(rl64(w[k], kEdTiles));
            }
            ms += g;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the descriptors are in the device ring
        // steps before tiles: a wave that sees a tile published then sees its
        // step copied (walk()'s upper bound is the mirror's step count)
        if (lane == 0) __hip_atomic_store(E.mirror + kMpSteps, hs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            __hip_atomic_store(E.mirror + kMpTiles, tiles, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // the grid's progress clock: waiting waves give up only when no new
            // step arrived for idle_ticks (timing each wave's own
            // wait let a wave holding a claim far ahead leave under steady light
            // traffic, stranding its tile)
            if (ms0 < hs) {
                __hip_atomic_store(E.mirror + kMpStamp, static_cast<uint64_t>(wall_clock64()), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            if (stop) __hip_atomic_store(E.mirror + kMpStop, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(E.mirror + kMpToken, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // Tile v is published, as far as the device mirror says (mid-tile: no
    // host poll here, so the poller's registers never meet a tile's).
    __device__ bool published(uint64_t v) {
        if (SCCSUM_HOT(v < pub)) return true;
#ifdef SCCSUM_AB_TIMELINE
        ++ab[2];
#endif
        pub = mload(kMpTiles);
        return v < pub;
    }
    // ... or after a poll of the host (a waiting wave: it holds no tile)
    __device__ bool published_polled(uint64_t v) {
        if (published(v)) return true;
        poll();
        pub = mload(kMpTiles);
        return v < pub;
    }
    // tile v (published) may start: its step has no dependency, or the step it
    // depends on is done (device copy of the done words; each slot only rises)
    __device__ bool dep_ready(uint64_t v) {
        walk(v);
        if (SCCSUM_HOT(sdep == 0 || sdep <= dep_seen)) return true;
        const uint32_t slot = static_cast<uint32_t>((sdep - 1) % kEngineCountSlots);
        uint64_t d = 0;
        if (lane == 0) d = __hip_atomic_load(E.sdone + 8u * slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        d = rfl64(d);
        if (d < sdep) return false;
        dep_seen = sdep;
        return true;
    }
    __device__ bool ready(uint64_t v) { return published(v) && dep_ready(v); }
    __device__ bool wait_ready(uint64_t v) {
        if (ready(v)) return true;
        flush();  // never wait holding counts: a step's completion may hang on them
        const uint64_t t0 = static_cast<uint64_t>(wall_clock64());
#ifdef SCCSUM_AB_TIMELINE
        ++ab[0];
        struct Slept {
            unsigned long long* a;
            uint64_t t0;
            __device__ ~Slept() { a[1] += static_cast<uint64_t>(wall_clock64()) - t0; }
        } slept{ab, t0};
#endif
        for (;;) {
            const uint64_t stop = mload(kMpStop);  // read before the tiles (the poller raises it after them)
            const bool pubd = published_polled(v);
            if (pubd) {
                // v's step waits on an older step: that always completes (its
                // tiles come before v in every group's claim order); the limit
                // only keeps a fault from hanging the device
                if (dep_ready(v)) return true;
                if (static_cast<uint64_t>(wall_clock64()) - t0 > E.dep_ticks) {
                    if (lane == 0) __hip_atomic_store(E.ctl + kEcError, kErrDepWait, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_SYSTEM);
                    return false;
                }
#ifdef SCCSUM_AB_DEP_SLEEP
                __builtin_amdgcn_s_sleep(SCCSUM_AB_DEP_SLEEP);
#else
                __builtin_amdgcn_s_sleep(32);  // ~0.9 us: a dependency ends with a step's last tiles
#endif
                continue;
            }
            if (stop) return false;  // stopped, and v lies past every published step
            // idle: no new step for idle_ticks, counted from this wait's start or
            // the poller's last new step, whichever is later
            const uint64_t now = static_cast<uint64_t>(wall_clock64());
            const uint64_t stamp = mload(kMpStamp);
            const uint64_t since = stamp > t0 ? stamp : t0;
            if (now > since && now - since > E.idle_ticks) {
                if (lane == 0) __hip_atomic_store(E.ctl + kEcError, kErrIdle, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_SYSTEM);
                return false;
            }
            // ~3.4 us (s_sleep 32 polled the mirror more and ran 32-packet steps
            // 13-29 % slower: profiles/r05_engine_small_steps.log)
            __builtin_amdgcn_s_sleep(127);
        }
    }
    __device__ uint64_t first() {
        const uint64_t v = claim(0);
        return wait_ready(v) ? v : end();
    }
    __device__ void set_cursor(uint64_t t, uint64_t w) {
        step = t;
        dw = w;
        sfirst = rl64(w, kEdFirst);
        slast = sfirst + static_cast<uint32_t>(rl64(w, kEdTiles));
        skind = rl64(w, kEdKind);
        sdep = rl64(w, kEdDep);
    }
    // tile v (published) -> the cursor on its step.  Claims only rise, so v's
    // step is the cursor's or a later one: the step after the cursor's first
    // (a wave's next tile is mostly there).  Steps are contiguous in tiles, so
    // that step starts where the cursor's ends, at or before v: its seal alone
    // says whether it holds v.  If it does, the step is not done, its slot not
    // reused, and every word of the descriptor read with the seal is its own.
    // (The whole index is checked too: a seal's 28-bit index could match a
    // step 2^28 later.)  Else engine_walk_far().
    __device__ bool walk(uint64_t v) {
        if (SCCSUM_HOT(step != ~0ull && v < slast)) return true;
#ifdef SCCSUM_AB_WALK_SEQ  // A/B only (a run shorter than its ring): round 5's walk, step by step
        while (step == ~0ull || v >= slast) {
            const uint64_t t = step + 1;
            set_cursor(t, __hip_atomic_load(E.dring + (t & E.ring_mask) * kEngineSlotWords + lane, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT));
        }
        return true;
#endif
#ifdef SCCSUM_AB_TIMELINE
        ++ab[3];
        const uint64_t w0 = static_cast<uint64_t>(wall_clock64());
        struct Walked {
            unsigned long long* a;
            uint64_t t0;
            __device__ ~Walked() { a[4] += static_cast<uint64_t>(wall_clock64()) - t0; }
        } walked{ab, w0};
#endif
        const uint64_t t = step + 1;  // (~0 + 1 = step 0, which starts at tile 0)
        const uint64_t w = __hip_atomic_load(E.dring + (t & E.ring_mask) * kEngineSlotWords + lane, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        if (SCCSUM_HOT(!seal_before(rl64(w, kEdStep), t, v) && rl64(w, kEdIndex) == t)) {
            set_cursor(t, w);
        } else {
            const WalkHit h = engine_walk_far(E.dring, E.ring_mask, E.mirror, E.ctl, t, v);
            set_cursor(rfl64(h.t), h.w);
        }
        return true;
    }
    // (v passed ready() / wait_ready(): the cursor is on its step)
    __device__ Ref ref(uint64_t v) {
        Ref r;
        r.kind = static_cast<uint32_t>(skind);
        const uint64_t t_in = v - sfirst;
        const uint32_t nq = static_cast<uint32_t>(rl64(dw, kEdNq));
        uint32_t q = 0;
        while (q + 1 < nq && t_in >= rl64(dw, kEdTile0 + q + 1)) ++q;
        r.B = static_cast<uint32_t>(rl64(dw, kEdTiles) >> 32);
        r.base = (t_in - rl64(dw, kEdTile0 + q)) * r.B;
        const uint32_t qw = kEdQueue + 8u * q;
        const uint64_t left = rl64(dw, qw + 7) - r.base;  // >= 1
        r.cnt = left < r.B ? static_cast<uint32_t>(left) : r.B;
        r.bytes = reinterpret_cast<const uint8_t*>(rl64(dw, qw + 0));
        r.bytes_len = rl64(dw, qw + 1);
        r.off = reinterpret_cast<const uint64_t*>(rl64(dw, qw + 2));
        r.len = reinterpret_cast<const uint32_t*>(rl64(dw, qw + 3));
        r.seed = reinterpret_cast<const uint32_t*>(rl64(dw, qw + 4));
        r.out = reinterpret_cast<uint16_t*>(rl64(dw, qw + 5));
        r.status = reinterpret_cast<uint8_t*>(rl64(dw, qw + 6));
        r.step = step;
        r.first = sfirst;
        r.last = slast;
        return r;
    }
    __device__ const uint8_t* bytes(const Ref& r) const { return r.bytes; }
    __device__ uint64_t bytes_len(const Ref& r) const { return r.bytes_len; }
    __device__ const uint64_t* off(const Ref& r) const { return r.off; }
    __device__ const uint32_t* len(const Ref& r) const { return r.len; }
    __device__ const uint32_t* seed(const Ref& r) const { return r.seed; }
    __device__ uint16_t* out(const Ref& r) const { return r.out; }
    __device__ uint8_t* status(const Ref& r) const { return r.status; }
    __device__ uint32_t tile_packets(const Ref& r) const { return r.B; }
    __device__ bool is_store(const Ref& r) const { return (r.kind & 0xffu) == kStepFillStore; }
    __device__ uint32_t fill_flags(const Ref& r, uint32_t) const { return (r.kind >> 8) & 0xffu; }
    __device__ uint32_t store_mode(const Ref& r) const { return r.kind >> 16; }
    // A tile's results are stored: count it for its step, per group (so no
    // counter sees more than its group's share).  A wave's tiles of one step
    // come in a row (claims rise), so it counts them itself and adds the count
    // once, when its tiles move on to a later step or before it waits: one
    // atomic round trip per step per wave instead of one per tile (per tile it
    // cost 18 % of cfg 2's step: profiles/r04g).  The step's last count resets
    // the counters and reports the step done.
    uint64_t pend_step = ~0ull, pend_first = 0, pend_last = 0;
    uint32_t pend = 0, pend_kind = 0;
#ifdef SCCSUM_AB_TIMELINE
    unsigned long long pend_t0 = 0, pend_t1 = 0;
#endif
    __device__ void flush() {
        if (pend == 0) return;
        const uint32_t k = pend;
        pend = 0;
#ifdef SCCSUM_AB_TIMELINE
        ++ab[5];
        struct Flushed {
            unsigned long long* a;
            uint64_t t0;
            __device__ ~Flushed() { a[6] += static_cast<uint64_t>(wall_clock64()) - t0; }
        } flushed{ab, static_cast<uint64_t>(wall_clock64())};
#endif
#ifdef SCCSUM_AB_TIMELINE
        if (lane == 0 && pend_step < kStepRec) {
            atomicMax(&g_step_grp[pend_step][grp], pend_t1);
            atomicMax(&g_step_xcd[pend_step][blockIdx.x & 7u][0], pend_t1);
            atomicMax(&g_step_xcd[pend_step][blockIdx.x & 7u][1], ~pend_t0);
        }
#endif
        if (lane != 0) return;
#ifdef SCCSUM_AB_FILLSTORE_NORELEASE
        if (false) {
#else
        if ((pend_kind & 0xffu) == kStepFillStore && !kStoreWT) {
#endif
            // the fields were stored plain: write them back from this XCD's L2
            // before the step can report (the host copies the frames out then)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        } else if (wt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the counted tiles' write-through result stores are done
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // their stores leave this XCD's L2 first
        }
        const uint64_t fg = pend_first + ((grp + kGroups - pend_first % kGroups) % kGroups);  // the group's first tile
        const uint32_t expect = fg < pend_last ? static_cast<uint32_t>((pend_last - 1 - fg) / kGroups + 1) : 0u;
        const uint32_t slot = static_cast<uint32_t>(pend_step % kEngineCountSlots);
        uint32_t* const c = E.counts + (slot * kGroups + grp) * kHeadStride;
        const uint32_t x = __hip_atomic_fetch_add(c, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (x + k != expect) return;
        __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t* const gd = E.gdone + slot * kHeadStride;
        const uint64_t ntl = pend_last - pend_first;
        const uint32_t groups = ntl < kGroups ? static_cast<uint32_t>(ntl) : kGroups;
        const uint32_t y = __hip_atomic_fetch_add(gd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (y + 1 != groups) return;
        __hip_atomic_store(gd, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the device's copy first (steps that depend on this one read it), then the host's
        __hip_atomic_store(E.sdone + 8u * slot, pend_step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (a ring of done words like the descriptors': the slot's value only
        // rises, and a value past s + 1 also says s is done)
        __hip_atomic_store(E.ctl + kEcDone + 8u * (pend_step & E.ring_mask), pend_step + 1, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
#ifdef SCCSUM_AB_TIMELINE
    __device__ void ab_stats(uint64_t wglob) {
        if (lane == 0 && wglob < kTimelineWaves)
            for (int i = 0; i < 8; ++i) g_engine_stats[wglob][i] = ab[i];
    }
#endif
    __device__ void retire(const Ref& r) {
        if (r.step != pend_step) {
            flush();
            pend_step = r.step;
            pend_first = r.first;
            pend_last = r.last;
            pend_kind = r.kind;
#ifdef SCCSUM_AB_TIMELINE
            pend_t0 = static_cast<uint64_t>(wall_clock64());
#endif
        }
        ++pend;
#ifdef SCCSUM_AB_TIMELINE
        pend_t1 = static_cast<uint64_t>(wall_clock64());
#endif
    }
};

// In-place fill, store half, for one frame of length L >= 20 at p: the values
// the generate half made (FILL phase C, *wp = IP | L4 << 16) go into the
// frame's fields.  Which fields is decided from the frame's own (unmodified)
// header exactly as the generate half decided it.  Field bytes of different
// frames never overlap, so the 2-byte stores need no coordination.
// kCoherent (the engine's store tiles, which share a running grid with the
// generate tiles that wrote *wp on other XCDs): the value and the header are
// read at agent scope, past this XCD's L2, and the fields are written through
// (sc0 sc1), so the host may copy the frames out once the step reports.
template <bool kCoherent>
__device__ __forceinline__ uint32_t fill_ld32(const uint32_t* q) {
    if constexpr (kCoherent) {  // (a global-space pointer: global_load, not flat_load, which also counts lgkm)
        return __hip_atomic_load(gld(q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        return *gld(q);
    }
}
// What the store half reads of one frame: its value word and header bytes
// 0..9 from the four dwords at the dword-aligned address at or below p (one
// 16-byte request instead of four byte loads).  (Issuing the offset, length
// and words loads together, two round trips instead of the three the compiler
// makes of this, ran the fill 0.8 % slower: r04zz.)  Loads and stores are two
// calls so a caller with several frames per lane issues every load first.
struct FillHead {
    uint32_t w, d0, d1, d2, d3;
};
template <bool kCoherent>
__device__ __forceinline__ FillHead fill_load(const uint8_t* p, const uint32_t* wp) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t* d = reinterpret_cast<const uint32_t*>(a & ~uintptr_t(3));
    FillHead h;
    h.w = fill_ld32<kCoherent>(wp);
    h.d0 = fill_ld32<kCoherent>(d);
    h.d1 = fill_ld32<kCoherent>(d + 1);
    h.d2 = fill_ld32<kCoherent>(d + 2);
    h.d3 = fill_ld32<kCoherent>(d + 3);
    return h;
}
// kCoherent: the ICMP type byte is read at agent scope; kWriteThrough: the
// fields are stored sc0 sc1 (else plain: the L2 merges a frame's two fields
// into one line write, and the engine releases a store step's fields once per
// wave, in flush)
template <bool kCoherent, bool kWriteThrough = false>
__device__ __forceinline__ void fill_apply(uint8_t* p, uint32_t L, const FillHead& h, uint32_t mode) {
    const uint32_t sh = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p) & 3u);
    const uint32_t w = h.w, d0 = h.d0, d1 = h.d1, d2 = h.d2, d3 = h.d3;
    auto hbyte = [&](uint32_t k) {
        const uint32_t b = sh + k;
        const uint32_t dw = b < 4u ? d0 : (b < 8u ? d1 : (b < 12u ? d2 : d3));
        return (dw >> (8u * (b & 3u))) & 0xffu;
    };
    const uint32_t ihl = hbyte(0) & 0xfu;
    const uint32_t ip_len = (hbyte(2) << 8) | hbyte(3);
    const uint32_t fragw = (hbyte(6) << 8) | hbyte(7);
    const uint32_t proto = hbyte(9);
    const uint32_t l4_off = 4u * ihl;
    const uint32_t l4_end = ip_len < L ? ip_len : L;
    // as frame_decode: malformed, an IP fragment, or ihl < 5 -> no L4 write
    const bool atomic = !(L < ip_len || l4_off > l4_end || (fragw & 0x1fffu) * 8u + l4_end > 65535u ||
                          (fragw & 0x3fffu) != 0u || ihl < 5u);
    const uint32_t l4_len = l4_off > l4_end ? 0u : l4_end - l4_off;
    if (mode & SCCSUM_FILL_IP) store_field<kWriteThrough>(p + 10, w);
    if (!atomic) return;
    if (mode & SCCSUM_FILL_L4) {
        const uint32_t fo = proto == 17u ? 6u : (proto == 6u ? 16u : 0u);
        if (fo != 0u && l4_len >= fo + 2u) store_field<kWriteThrough>(p + l4_off + fo, w >> 16);
    }
    if ((mode & SCCSUM_FILL_ICMP_ECHO) && proto == 1u && l4_len >= 8u) {
        uint8_t* ih = p + l4_off;
        const uintptr_t ia = reinterpret_cast<uintptr_t>(ih);
        const uint32_t type = (fill_ld32<kCoherent>(reinterpret_cast<const uint32_t*>(ia & ~uintptr_t(3))) >>
                               (8u * static_cast<uint32_t>(ia & 3u))) & 0xffu;
        if (type == 8u) {  // echo_request -> echo_reply, code 0, checksum (ip.cc:469-474)
            store_field<kWriteThrough>(ih, 0u);
            store_field<kWriteThrough>(ih + 2, w >> 16);
        }
    }
}

template <int U, bool IPV4, bool FILL, bool PIPE, bool PLATE, class Src>
__device__ __forceinline__ void flat_body(Src& src, const uint32_t flags, const RssParams& rss) {
    static_assert(!FILL || IPV4, "in-place generate is a frames mode");
    constexpr uint32_t C = kWave * U;  // units per chunk
    constexpr uint32_t kLdsUnits = C;
    constexpr int kHead = FILL ? 4 : (IPV4 ? 3 : 1);
    using Ref = typename Src::Ref;
    const bool short_chunks = (flags & kFlagFullChunks) == 0;
    // a run's streamed extent starts on a 64 / 128-byte boundary (clamped to
    // the batch's first unit), so each 1 KiB load row covers whole lines
    const uint32_t ra_code = (flags >> kRunAlignShift) & 3u;
    const uint64_t ra_mask = ra_code == 0 ? 0ull : (ra_code == 1 ? 3ull : 7ull);
    const bool raw = !IPV4 && (flags & kFlagRaw);
    __shared__ u32x4 ubuf_all[kWavesPerBlock][kLdsUnits];
    __shared__ uint32_t pbuf_all[kWavesPerBlock][kLdsUnits];
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    u32x4* ubuf = ubuf_all[wv];
    uint32_t* pbuf = pbuf_all[wv];
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
    const uint32_t vo = 16u * lane;
    const uint64_t wglob = static_cast<uint64_t>(xcd_block_id()) * kWavesPerBlock + wv;
    src.init(wglob, nwaves, lane);
    const uint64_t ntiles = src.end();
    auto next_tile = [&](uint64_t prev) -> uint64_t { return src.claim(prev); };
    // Two-deep tile pipeline: while tile t streams, the plan (offset, length,
    // seed) of the next tile is already loading and the tile after it is being
    // dequeued, so no tile starts on an exposed metadata or atomic round trip.
    // Every wave still makes exactly one failing dequeue (the counter reset
    // relies on it).  (One tile ahead instead lost: profiles/r04_ab_dequeue_depth.log.)
    uint64_t t = src.first();
    // A launch's first claim (tile t1) is issued after the first tile's plan
    // loads and read back after its derive, so the two round trips of a
    // wave's start overlap (the late-claim forms; see the tile loop).
    constexpr bool kLate = !PIPE || PLATE;
    constexpr bool kLateStart = kLate && !Src::kEngine;
    uint64_t t1 = (!kLateStart && t < ntiles) ? next_tile(t) : ntiles;
    auto plan_load = [&](const Ref& tr, bool valid, uint64_t& o_, uint32_t& L_, uint32_t& sd_) {
        const uint32_t c_ = valid ? tr.cnt : 0u;
        const uint64_t q_ = tr.base + (lane < c_ ? lane : 0);
        o_ = gld(src.off(tr))[q_];
        L_ = lane < c_ ? gld(src.len(tr))[q_] : 0u;
        const uint32_t* sq = IPV4 ? nullptr : src.seed(tr);
        sd_ = sq != nullptr ? gld(sq)[q_] : 0u;
    };
    // ---- A: a tile's per-lane packet plan and its runs: lane j starts a new
    // run unless packet j-1 and j both take part and j's span starts at most
    // kGapUnits past j-1's end and ends no earlier (so a run's extent is
    // [fu of its first, lu of its last])
    struct Tile {
        Ref ref;
        uint64_t base, o, a0, fu, lu, starts, streamed;
        uint32_t cnt, L, sd, head, nunits;
        bool mine, range_bad, short_frame, huge, fast, part;
    };
    auto derive = [&](const Ref& tr, uint64_t o_, uint32_t L_, uint32_t sd_) {
        Tile c;
        c.ref = tr;
        c.base = tr.base;
        c.cnt = tr.cnt;
        c.mine = lane < c.cnt;
        c.o = o_;
        c.L = L_;
        c.sd = sd_;
        const uint64_t bytes_len = src.bytes_len(tr);
        c.range_bad = c.o > bytes_len || c.L > bytes_len - c.o;
        c.short_frame = IPV4 && c.L < 20;
        c.huge = c.L > kExactMax;
        const uint8_t* ptr = src.bytes(tr) + (c.range_bad ? 0 : c.o);
        c.head = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(ptr) & 15u);
        c.a0 = reinterpret_cast<uint64_t>(ptr - c.head);
        c.fast = c.mine && !c.range_bad && !c.short_frame && !c.huge;
        c.nunits = (c.fast && c.L) ? (c.head + c.L + 15u) >> 4 : 0u;
        c.part = c.nunits != 0;
        c.fu = c.a0 >> 4;
        c.lu = c.fu + c.nunits - 1;
        const int pl = static_cast<int>(lane == 0 ? 0 : lane - 1);
        const uint64_t pfu =
            (static_cast<uint64_t>(static_cast<uint32_t>(__shfl(static_cast<int>(c.fu >> 32), pl))) << 32) |
            static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(c.fu)), pl));
        const uint64_t plu =
            (static_cast<uint64_t>(static_cast<uint32_t>(__shfl(static_cast<int>(c.lu >> 32), pl))) << 32) |
            static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(c.lu)), pl));
        const bool ppart = __shfl(static_cast<int>(c.part), pl) != 0;
        const bool joins = lane != 0 && c.part && ppart && c.fu >= pfu && c.lu >= plu && c.fu <= plu + kGapUnits;
        c.starts = __ballot(c.mine && !joins) | (c.cnt < 64 ? (1ull << c.cnt) : 0ull);
        c.streamed = c.starts & __ballot(c.part);  // runs that stream bytes start at a lane that takes part
        return c;
    };
    // Run [k, k2) of tile c: its extent's first unit F and unit count.
    struct Run {
        uint32_t k, k2, ext;
        uint64_t F;
    };
    auto run_of = [&](const Tile& c, uint32_t k) {
        Run rn;
        rn.k = k;
        const uint64_t after = c.starts & ~((2ull << k) - 1ull);  // k < 64; bit cnt is the sentinel
        rn.k2 = after ? static_cast<uint32_t>(__builtin_ctzll(after)) : c.cnt;
        // (readlane returns int: widen through uint32_t, never sign-extend an address half)
        const uint32_t Fhi = __builtin_amdgcn_readlane(static_cast<uint32_t>(c.fu >> 32), k);
        const uint32_t Flo = __builtin_amdgcn_readlane(static_cast<uint32_t>(c.fu), k);
        rn.F = (static_cast<uint64_t>(Fhi) << 32) | Flo;
        const uint64_t lo_u = reinterpret_cast<uint64_t>(src.bytes(c.ref)) >> 4;  // the batch's first unit
        const uint64_t Fa = rn.F & ~ra_mask;
        rn.F = Fa >= lo_u ? Fa : lo_u;  // (F >= lo_u: the run's first packet lies in the batch)
        const uint32_t Llo = __builtin_amdgcn_readlane(static_cast<uint32_t>(c.lu), rn.k2 - 1);
        rn.ext = Llo - static_cast<uint32_t>(rn.F) + 1u;  // units in the run's extent
        return rn;
    };
    auto run_rsrc = [&](const Run& rn) { return rsrc(reinterpret_cast<const uint8_t*>(rn.F << 4), 16u * rn.ext); };
    // a chunk's loads: R <= U rows of 64 units
    auto load = [&](const __amdgpu_buffer_rsrc_t& r, uint32_t g, auto& v) {
        constexpr int R = std::extent<std::remove_reference_t<decltype(v)>>::value;
#pragma unroll
        for (int u = 0; u < R; ++u)
            v[u] = __builtin_amdgcn_raw_buffer_load_b128(r, static_cast<int>(16u * g + vo + 1024u * u), 0, kNT);
    };

    uint64_t o_n = 0;
    uint32_t L_n = 0, sd_n = 0;
    // the next tile's Ref, from its plan to its derive (an engine's Ref
    // resolves its step once)
    Ref r_n{};
    if (Src::kEngine) {
        if (t < ntiles) {
            r_n = src.ref(t);
            plan_load(r_n, true, o_n, L_n, sd_n);
        }
    } else {
        r_n = src.ref(t < ntiles ? t : 0);
        plan_load(r_n, t < ntiles, o_n, L_n, sd_n);
    }
    typename Src::Claim c1{};
    bool c1p = false;
    if (kLateStart && t < ntiles) {
        c1 = src.claim_issue(t);
        c1p = true;
    }
    Tile cur{};
    // A tile's results into out / status.
    auto put = [&](const Ref& r, uint64_t bse, bool mn, uint32_t wd, uint32_t sv) {
        uint16_t* const out = src.out(r);
        uint8_t* const status = src.status(r);
#ifdef SCCSUM_AB_NOSTORE
        // A/B only (tools/build_ab.sh): the result stores left out of the
        // stream — kept behind a test no lane passes, so nothing is optimised away
        if (mn && wd == 0x5EA57A2Cu && sv == 0x77u) {
#else
        if (mn) {
#endif
            // the policy applies to an array whose tile part spans >= 128 B
            // (two lines); a smaller part is stored plain, so that the L2
            // merges it with its neighbour tiles' parts into whole lines
            // (nt parts of a line leave as separate partial writes: cfg 4's
            // 1-segment tiles wrote 107 B per segment and ran 8 % slower)
            // (an engine's results are written through, sc0 sc1: the host may read
            // a step's results as soon as the step reports, while the grid runs)
            const uint32_t B = src.tile_packets(r);
            const bool wt = Src::kEngine && (flags & kFlagEngineWT);
            const uint32_t pol = wt ? 3u : (flags >> kOutPolicyShift) & 7u;
            const uint32_t pol_out = wt || B * (IPV4 ? 4u : 2u) >= 128u ? pol : 0u;
            const uint32_t pol_st = wt || B >= 128u ? pol : 0u;
            if (IPV4) {
                if (out) tile_store(reinterpret_cast<uint32_t*>(out) + bse, lane, wd, pol_out);
            } else {
                tile_store(out + bse, lane, static_cast<uint16_t>(wd), pol_out);
            }
            if (status) tile_store(status + bse, lane, static_cast<uint8_t>(sv), pol_st);
        }
    };
#ifdef SCCSUM_AB_TIMELINE
    const unsigned long long tl_start = wall_clock64();
    unsigned long long tl_first = 0, tl_tiles = 0;
#endif
    while (t < ntiles) {
#ifdef SCCSUM_AB_TIMELINE
        ++tl_tiles;
#endif
        // The claim of the tile after next: issued after this tile's last loads
        // (below) and read back after the tile, so its round trip overlaps the
        // last chunk's.  Read back at once, where it is issued, it stalled the
        // wave before every tile's first loads: cfg 2 +0.5 %, cfg 3 +1.3 %,
        // cfg 4 +0.6-2.3 % this way (profiles/r04_engine_groups.log).  The
        // atomic optimizer is off (build.py): it would read the atomic back
        // where it is issued.
        // The chunk-in-flight forms (PIPE, small launches) issue it after their
        // last real chunk load (PLATE) only for launches of 1 KiB+ packets and
        // 256 MiB+: 2 x 131 072 x 1500 B frames ran 5.5-6 % faster that way,
        // 262 144 Zipf frames 4.7 % and 2 x 32 768 frames 3.5 % slower
        // (profiles/r04_engine_groups.log, r05e-r05f).  Otherwise they read it
        // back at once.
        uint64_t t2 = ntiles;
        if (!kLate && t1 < ntiles) t2 = next_tile(t1);
        cur = derive(r_n, o_n, L_n, sd_n);
        if (kLateStart && c1p) {  // the launch's first claim (above)
            t1 = rfl64(src.claim_resolve(c1));
            c1p = false;
        }
        const bool claiming = t1 < ntiles;
        bool issued = false;
        typename Src::Claim c2{};
        auto issue = [&]() {
            if (kLate && claiming && !issued) {
                c2 = src.claim_issue(t1);
                issued = true;
            }
        };
        // an engine's next tile may belong to a step not published yet: its plan
        // then waits until this tile is done (a wave never waits holding work)
        bool planned = false;
        if (t1 < ntiles && src.ready(t1)) {
            r_n = src.ref(t1);
            plan_load(r_n, true, o_n, L_n, sd_n);
            planned = true;
        }
        const uint64_t base = cur.base;
        const bool mine = cur.mine;
        const uint32_t L = cur.L, sd = cur.sd, head = cur.head, nunits = cur.nunits;
        const uint64_t a0 = cur.a0;
        const bool range_bad = cur.range_bad, short_frame = cur.short_frame, huge = cur.huge, fast = cur.fast;

        // the tile's fill flags: a launch's are the kernel's; an engine's come
        // with its step (a FILL engine runs verify and generate steps too)
        const uint32_t ff = FILL ? src.fill_flags(cur.ref, flags) : 0u;
        const bool fill_tile = FILL && (ff & kFillFlags) != 0u;
        const bool fill_ip = fill_tile && (ff & kFlagFillIp);
        const bool fill_l4 = fill_tile && (ff & kFlagFillL4);
        const bool fill_icmp = fill_tile && (ff & kFlagFillIcmp);
        // an engine fill's store tile: one frame per lane, nothing streamed
        const bool store_tile = Src::kEngine && FILL && src.is_store(cur.ref);
#ifdef SCCSUM_AB_NOFILLSTORE
        if (store_tile) {  // A/B only (tools/build_ab.sh): a store tile does nothing (the step's barrier alone)
            issue();
        } else
#endif
        if (store_tile) {
            issue();  // the claim of the tile after next
            // frames base + lane + 64 j, j < J: every load of the tile issues
            // before its first store (one frame per lane left the store phase
            // with a quarter of the frames in flight that the launch's store
            // pass keeps, 8 waves per SIMD against the engine's 2)
            constexpr int J = static_cast<int>(kStoreTilePackets) / kWave;
            uint8_t* const sb = const_cast<uint8_t*>(src.bytes(cur.ref));
            const uint64_t slen = src.bytes_len(cur.ref);
            const uint64_t* const soffs = src.off(cur.ref);
            const uint32_t* const slens = src.len(cur.ref);
            const uint32_t* const swords = reinterpret_cast<const uint32_t*>(src.out(cur.ref));
            uint64_t so[J];
            uint32_t sl[J];
            bool sv[J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const uint32_t k = lane + static_cast<uint32_t>(kWave * j);
                sv[j] = k < cur.cnt;
                const uint64_t q = base + (sv[j] ? k : 0u);
                so[j] = gld(soffs)[q];
                sl[j] = sv[j] ? gld(slens)[q] : 0u;
            }
            FillHead fh[J];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                sv[j] = sv[j] && so[j] <= slen && sl[j] <= slen - so[j] && sl[j] >= 20u;
                if (sv[j]) fh[j] = fill_load<true>(sb + so[j], swords + base + lane + kWave * j);
            }
            const uint32_t smode = src.store_mode(cur.ref);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (sv[j]) fill_apply<true, kStoreWT>(sb + so[j], sl[j], fh[j], smode);
            }
        } else {
        // ---- B: stream each run's extent
        u32x4 hs[4] = {u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}, u32x4{0, 0, 0, 0}};
        u32x4 hl = u32x4{0, 0, 0, 0};
        uint32_t pst = 0, pend = 0;
        uint64_t rem = cur.streamed;
        while (rem != 0) {
            const Run rn = run_of(cur, static_cast<uint32_t>(__builtin_ctzll(rem)));
            rem &= rem - 1;
            const uint32_t k = rn.k, k2 = rn.k2, ext = rn.ext;
            const uint64_t F = rn.F;
            const auto r = run_rsrc(rn);
            const bool cap = lane >= k && lane < k2;
            const int rf = cap ? static_cast<int>(static_cast<uint32_t>(cur.fu - F)) : -0x40000000;
            const int rl = cap ? static_cast<int>(static_cast<uint32_t>(cur.lu - F)) : -0x40000000;
            uint32_t carry = 0;
            const bool last_run = rem == 0;
            // one chunk = R <= U rows of 64 units: unit sums, scanned, parked
            // in LDS with the units; packet lanes pick up what falls in it
            auto chunk = [&](uint32_t g, const auto& v) {
                constexpr int R = std::extent<std::remove_reference_t<decltype(v)>>::value;
                constexpr uint32_t CR = kWave * R;  // units in this chunk
                uint32_t x[R];
#pragma unroll
                for (int u = 0; u < R; ++u) x[u] = sad4(v[u], 0u);
                wave_scan_n<R>(x);
#pragma unroll
                for (int u = 0; u < R; ++u) {
                    pbuf[kWave * u + lane] = carry + x[u];
                    ubuf[kWave * u + lane] = v[u];
                    carry += __builtin_amdgcn_readlane(x[u], 63);
                }
                __builtin_amdgcn_wave_barrier();
                const int a = rf - static_cast<int>(g);
                if (static_cast<uint32_t>(a) < CR) {
                    const u32x4 w = ubuf[a];
                    pst = pbuf[a] - sad4(w, 0u);  // prefix just before the first unit
                    hs[0] = w;
                }
#pragma unroll
                for (int j = 1; j < kHead; ++j) {
                    if (static_cast<uint32_t>(a + j) < CR) hs[j] = ubuf[a + j];
                }
                const int b = rl - static_cast<int>(g);
                if (static_cast<uint32_t>(b) < CR) {
                    pend = pbuf[b];
                    hl = ubuf[b];
                }
                __builtin_amdgcn_wave_barrier();  // this chunk's LDS reads precede the next chunk's writes
#ifdef SCCSUM_AB_TIMELINE
                if (tl_first == 0) tl_first = wall_clock64();
#endif
            };
            if (PIPE) {
                u32x4 va[U], vb[U];
                const uint32_t lastg = last_run ? ((ext - 1u) / C) * C : ~0u;  // the run's last real chunk
                load(r, 0, va);
                if (lastg == 0u) issue();
                for (uint32_t g = 0; g < ext; g += 2 * C) {
                    load(r, g + C, vb);
                    if (g + C == lastg) issue();
                    chunk(g, va);
                    load(r, g + 2 * C, va);
                    if (g + 2 * C == lastg) issue();
                    chunk(g + C, vb);
                }
            } else {
                // a run's last chunk loads and scans only the rows its units
                // reach (U / 8 .. U): a run of one 1500 B frame in an mbuf slot
                // is 2 rows, not 16 (packed layouts: no change,
                // profiles/r02_ab_short_chunks.log)
                for (uint32_t g = 0; g < ext; g += C) {
                    const uint32_t left = ext - g;
                    const bool last = last_run && left <= C;  // the tile's last loads: then the claim
#ifndef SCCSUM_AB_NOREMROW
                    if (left > C && left <= C + static_cast<uint32_t>(kWave)) {
                        // a full chunk and a remainder of at most one row (a 65 535 B
                        // segment's extent is 4 097-4 104 units): the row is loaded with
                        // the chunk, so it costs no round trip of its own
                        u32x4 v[U];
                        u32x4 t[1];
                        load(r, g, v);
                        load(r, g + C, t);
                        if (last_run) issue();
                        chunk(g, v);
                        chunk(g + C, t);
                        break;
                    }
#endif
                    if (!short_chunks || left > C / 2) {
                        u32x4 v[U];
                        load(r, g, v);
                        if (last) issue();
                        chunk(g, v);
                    } else if (left > C / 4) {
                        u32x4 v[U / 2];
                        load(r, g, v);
                        if (last) issue();
                        chunk(g, v);
                    } else if (U < 8 || left > C / 8) {
                        u32x4 v[U / 4];
                        load(r, g, v);
                        if (last) issue();
                        chunk(g, v);
                    } else {
                        u32x4 v[U >= 8 ? U / 8 : 1];
                        load(r, g, v);
                        if (last) issue();
                        chunk(g, v);
                    }
                }
            }
        }
        issue();  // (a tile that streamed nothing, or the chunk-in-flight forms)
        const uint32_t res = pend - pst;  // sum of the packet's units, mod 2^32
        if (IPV4 && huge && mine && !range_bad) {  // not streamed (phase D redoes its sum): head units from the frame
            const auto* hu = gld(reinterpret_cast<const u32x4*>(a0));
#pragma unroll
            for (int j = 0; j < kHead; ++j) hs[j] = hu[j];
        }

        // ---- C: lane i finishes packet i
        // ICMP echo fill: the reply's type, code and checksum are 0, so its sum
        // is the request's message after the first 4 bytes (and a message that
        // is all zeros there sums to 0, checksum 0xffff, like the reference)
        const bool icmp_lane = FILL && fill_icmp && ((header_dword(hs, head, 2) >> 8) & 0xffu) == 1u;
        const int skip = icmp_lane ? 4 : 0;
        const int rs0 = static_cast<int>(head) + (IPV4 ? 20 + skip : 0);
        const int re0 = static_cast<int>(head + L);
        const int lastu16 = 16 * (static_cast<int>(nunits) - 1);
        uint32_t excl = unit_part(hs[0], 0, rs0);
        if (IPV4) excl += unit_part(hs[1], 0, rs0 - 16) + unit_part(hs[2], 0, rs0 - 32);
        excl += unit_part(hl, re0 - lastu16, 16);
        const uint32_t kept = nunits ? res - excl : 0u;
        uint32_t S = fold16(kept);
        if (head & 1u) S = swap16(S);
        uint32_t word = 0, st = 0;
        bool slow = huge && mine && !range_bad;
        uint32_t ipc = 0, pseudo = 0, fpos = 0;
        int srs = 0, sre = 0;
#ifdef SCCSUM_AB_NOFINISH
        constexpr bool kFinish = false;  // A/B only (tools/build_ab.sh): no IPv4 decode / fill plan in phase C
#else
        constexpr bool kFinish = true;
#endif
        if (IPV4 && kFinish) {
            const uint32_t h0 = header_dword(hs, head, 0), h1 = header_dword(hs, head, 1);
            const uint32_t h2 = header_dword(hs, head, 2), h3 = header_dword(hs, head, 3);
            const uint32_t h4 = header_dword(hs, head, 4);
            const FrameDecode D = frame_decode(h0, h1, h2, h3, h4, L);
            ipc = ~fold16(static_cast<uint64_t>(h0) + h1 + (fill_tile ? h2 & 0xffffu : h2) + h3 + h4) & 0xffffu;
            const uint32_t ihl = D.ihl, l4_off = D.l4_off, l4_len = D.l4_len;
            st = D.st;
            pseudo = D.pseudo;
            slow = slow || (fast && (ihl != 5u || D.ip_len != L));
            srs = static_cast<int>(head + l4_off) + skip;
            sre = static_cast<int>(head + l4_off + l4_len);
            if (rss.hash != nullptr) {  // fused RSS: the 4-tuple is already in registers
                const uint32_t h5 = header_dword(hs, head, 5);
                uint32_t pl = h5;
                if (rss.mode != SCCSUM_RSS_DISPATCH && ihl != 5u && l4_off + 4u <= L && mine && !range_bad) {
                    const uint8_t* q = reinterpret_cast<const uint8_t*>(a0) + head + l4_off;  // options: rare
                    pl = static_cast<uint32_t>(q[0]) | (static_cast<uint32_t>(q[1]) << 8) |
                         (static_cast<uint32_t>(q[2]) << 16) | (static_cast<uint32_t>(q[3]) << 24);
                }
                uint32_t hv = 0;
                rss_ipv4(rss, h0, h1, h2, h3, h4, h5, pl, L, hv);
                if (mine) rss.hash[base + lane] = (range_bad || short_frame) ? 0u : hv;  // one queue with RSS
            }
            if (fill_tile) {
                // L4 writers never touch an IP fragment, a malformed frame, or a
                // frame whose ihl is below 5 (its L4 header would overlap the
                // 20-byte IP header: no reference writer builds one, ip.cc:249)
                const bool atomic = (st & (SCCSUM_ST_MALFORMED | SCCSUM_ST_IPFRAG)) == 0u && ihl >= 5u;
                uint32_t fo = 0;
                if (fill_l4 && (D.proto == 17u || D.proto == 6u)) fo = D.proto == 17u ? 6u : 16u;
                if (icmp_lane && atomic && l4_len >= 8u) {  // get_header<icmp_hdr>(0): 8 bytes (ip.hh:143-156)
                    uint32_t type = 0;
                    if (ihl == 5u) {
                        type = header_dword(hs, head, 5) & 0xffu;
                    } else if (mine && !range_bad) {  // options: the type byte from memory (rare)
                        type = reinterpret_cast<const uint8_t*>(a0)[head + l4_off];
                    }
                    fo = type == 8u ? 2u : 0u;  // echo_request only (ip.cc:466)
                }
                const bool has_field = fo != 0u && atomic && l4_len >= fo + 2u;
                fpos = has_field ? head + l4_off + fo : 0u;
                uint32_t rr;
                if (icmp_lane) {
                    rr = ~S & 0xffffu;
                } else {
                    uint32_t fv = 0;
                    if (has_field && !slow) {  // ihl == 5: frame bytes 26-27 (UDP) / 36-37 (TCP)
                        fv = fo == 6u ? header_dword(hs, head, 6) >> 16 : header_dword(hs, head, 9) & 0xffffu;
                    }
                    rr = ~fold16(static_cast<uint64_t>(S) + pseudo + (~fv & 0xffffu)) & 0xffffu;
                }
                word = (fill_ip ? ipc : 0u) | (has_field ? rr << 16 : 0u);
                st |= (fill_ip ? SCCSUM_ST_OK : 0u) | (has_field ? SCCSUM_ST_L4_OK : 0u);
                slow = slow && has_field;  // nothing else needs the exact sum
            } else {
                const uint32_t rr = ~fold16(static_cast<uint64_t>(S) + pseudo) & 0xffffu;
                word = frame_word(ipc, rr, st);
                st = frame_status(ipc, rr, st);
                slow = slow && (st & SCCSUM_ST_IPFRAG) == 0u;  // a fragment claims no L4 value
            }
        } else {
            const uint32_t rr = raw ? S : ~fold16(static_cast<uint64_t>(S) + swap16(fold16(sd))) & 0xffffu;
            word = rr;
            st = (!raw && rr == 0) ? SCCSUM_ST_OK : 0u;
        }
        if (range_bad) {
            word = 0;
            st = SCCSUM_ST_RANGE;
        } else if (short_frame) {
            word = 0;
            st = SCCSUM_ST_MALFORMED;
        }

        // ---- D: exact redo of the packets the fast path could not take
        uint64_t todo = __ballot(slow);
        while (todo) {
            const uint32_t j = static_cast<uint32_t>(__builtin_ctzll(todo));
            todo &= todo - 1;
            const uint32_t jlo = __builtin_amdgcn_readlane(static_cast<uint32_t>(a0), j);
            const uint32_t jhi = __builtin_amdgcn_readlane(static_cast<uint32_t>(a0 >> 32), j);
            const uint8_t* ja0 = reinterpret_cast<const uint8_t*>((static_cast<uint64_t>(jhi) << 32) | jlo);
            const uint32_t jhead = __builtin_amdgcn_readlane(head, j);
            uint64_t rs, re;
            if (IPV4) {
                rs = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(srs), j));
                re = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(sre), j));
            } else {
                rs = jhead;
                re = static_cast<uint64_t>(jhead) + static_cast<uint32_t>(__builtin_amdgcn_readlane(L, j));
            }
            uint32_t SJ = exact_range_sum(ja0, rs, re, lane);
            if (jhead & 1u) SJ = swap16(SJ);
            if (lane == j) {
                if (IPV4 && fill_tile) {
                    uint32_t rr = ~SJ & 0xffffu;  // ICMP echo: the message after type, code, checksum
                    if (!icmp_lane) {
                        const uint8_t* fp = reinterpret_cast<const uint8_t*>(a0) + fpos;
                        const uint32_t fv = static_cast<uint32_t>(fp[0]) | (static_cast<uint32_t>(fp[1]) << 8);
                        rr = ~fold16(static_cast<uint64_t>(SJ) + pseudo + (~fv & 0xffffu)) & 0xffffu;
                    }
                    word = (word & 0xffffu) | (rr << 16);
                } else if (IPV4) {
                    const uint32_t rr = ~fold16(static_cast<uint64_t>(SJ) + pseudo) & 0xffffu;
                    word = ipc | (rr << 16);
                    st = (st & ~SCCSUM_ST_L4_OK) | (rr == 0 ? SCCSUM_ST_L4_OK : 0u);
                } else {
                    const uint32_t rr = raw ? SJ : ~fold16(static_cast<uint64_t>(SJ) + swap16(fold16(sd))) & 0xffffu;
                    word = rr;
                    st = (!raw && rr == 0) ? SCCSUM_ST_OK : 0u;
                }
            }
        }

        put(cur.ref, base, mine, word, st);
        // A single-pass fill (kFlagFillNow: small fills, sccsum_ipv4_fill and
        // sccsum_engine_submit_fill) stores the fields from the tile, after
        // every read of it: the status says which (ST_OK the IP field,
        // ST_L4_OK the L4 or ICMP one; RANGE / MALFORMED frames none).  A
        // store inside the read stream costs more than the store pass at 1 M
        // frames (§5.6); a small fill is bound by latency instead, and one
        // pass saves the store kernel's launch or the store step's wait.
        // (The engine writes them through, as its store tiles do.)
        if (FILL && fill_tile && (ff & kFlagFillNow) && mine) {
            uint8_t* const f0 = reinterpret_cast<uint8_t*>(a0);
            if (st & SCCSUM_ST_OK) store_field<Src::kEngine>(f0 + head + 10, word);
            if (st & SCCSUM_ST_L4_OK) {
                if (icmp_lane) store_field<Src::kEngine>(f0 + fpos - 2, 0u);  // echo reply: type 0, code 0
                store_field<Src::kEngine>(f0 + fpos, word >> 16);
            }
        }
        // (readfirstlane: the compiler otherwise loses the tile number's
        // uniformity across the issue branches and reads the next tile's queue
        // fields with vector loads, 8 more per tile)
        }  // (not a store tile)
        if (kLate && claiming) t2 = rfl64(src.claim_resolve(c2));
        src.retire(cur.ref);
        if (Src::kEngine && t1 < ntiles && !planned) {
            if (src.wait_ready(t1)) {
                r_n = src.ref(t1);
                plan_load(r_n, true, o_n, L_n, sd_n);
            } else {
                t1 = t2 = ntiles;  // stopped: t1 (and t2 after it) lie past every step
            }
        }
        t = t1;
        t1 = t2;
    }
#ifdef SCCSUM_AB_TIMELINE
    if (lane == 0 && wglob < kTimelineWaves) {
        g_timeline[wglob][0] = tl_start;
        g_timeline[wglob][1] = tl_first;
        g_timeline[wglob][2] = wall_clock64();
        g_timeline[wglob][3] = tl_tiles;
    }
    if constexpr (Src::kEngine) src.ab_stats(wglob);
#endif
}

template <int U, bool IPV4, bool FILL, bool PIPE, bool PLATE = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(U >= 16 ? 2 : 3))) void csum_flat_kernel(
    const Queues Q, uint32_t B, uint32_t* __restrict__ heads, uint32_t* __restrict__ done, uint32_t ticket,
    uint32_t flags, const RssParams rss) {
    QueueSrc src(Q, B, heads, done, ticket);
    flat_body<U, IPV4, FILL, PIPE, PLATE>(src, flags, rss);
}

// FILL: an engine that also takes fill steps (sccsum_engine_submit_fill)
template <int U, bool IPV4, bool FILL = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(U >= 16 ? 2 : 3))) void csum_engine_kernel(
    const EngineArgs E, uint32_t flags) {
    EngineSrc src(E, flags);
    flat_body<U, IPV4, FILL, false, false>(src, flags, RssParams{});
}

// Fragment lists (checksummer::sum(const packet&), src/net/ip_checksum.cc:64-68):
// stage 1 = the span kernel in raw mode gives every fragment's folded sum
// relative to the fragment's own start; here one thread per packet walks its
// fragments in order and byte-swaps each sum whose fragment starts at an odd
// packet-relative offset — the reference's `odd` carry (ip_checksum.cc:33-36,
// 52) — then adds the seed and complements.
__global__ __launch_bounds__(kBlock) void frag_combine_kernel(const uint32_t* __restrict__ frag_len, uint64_t nfrag,
                                                               const uint32_t* __restrict__ pkt_first,
                                                               const uint16_t* __restrict__ raw,
                                                               const uint8_t* __restrict__ raw_status,
                                                               const uint32_t* __restrict__ seed,
                                                               uint16_t* __restrict__ out,
                                                               uint8_t* __restrict__ status, uint64_t n) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t f0 = pkt_first[i], f1 = pkt_first[i + 1];
    bool bad = f1 < f0 || f1 > nfrag;
    const uint64_t f_end = bad ? f0 : f1;
    uint64_t S = 0;
    uint32_t par = 0;
    // no exit on a bad fragment inside the loop: its trip count then depends
    // on no loaded value, so the loads of all the packet's fragments issue
    // back to back instead of one round trip per fragment (a 5-fragment
    // packet's walk was ~5 us of latency)
#pragma unroll 4
    for (uint64_t j = f0; j < f_end; ++j) {
        const uint32_t t = raw[j];
        bad = bad || (raw_status[j] & SCCSUM_ST_RANGE) != 0;
        S += par ? swap16(t) : t;
        par ^= frag_len[j] & 1u;
    }
    const uint32_t r = ~fold16(fold16(S) + static_cast<uint64_t>(swap16(fold16(seed ? seed[i] : 0u)))) & 0xffffu;
    out[i] = bad ? uint16_t(0) : static_cast<uint16_t>(r);
    if (status) status[i] = bad ? SCCSUM_ST_RANGE : (r == 0 ? SCCSUM_ST_OK : 0u);
}

// In-place fill, second pass: store the values the flat kernel generated
// (FILL instantiation, words[i] = IP | L4 << 16) into the frames' fields.
// One thread per frame; which fields it writes is decided from the frame's
// own (unmodified) header exactly as the first pass decided it.  The stores
// run as a pass of their own, after the read stream: interleaved with the
// stream the same stores cost ~100 us per 1 M frames, as their own pass
// ~70-90 us (HBM read/write turnarounds; tools/dev/store_probe.hip,
// DESIGN.md §5.6).  Field bytes of different frames never overlap, so the
// 2-byte stores need no coordination.
__global__ __launch_bounds__(kBlock) void fill_store_kernel(uint8_t* __restrict__ bytes, uint64_t bytes_len,
                                                            const uint64_t* __restrict__ off,
                                                            const uint32_t* __restrict__ len,
                                                            const uint32_t* __restrict__ words, uint64_t n,
                                                            uint32_t mode) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = off[i];
    const uint32_t L = len[i];
    if (o > bytes_len || L > bytes_len - o || L < 20u) return;
#ifdef SCCSUM_AB_FILLSTORE_LAUNCH_WT
    fill_apply<false, true>(bytes + o, L, fill_load<false>(bytes + o, words + i), mode);
#else
    fill_apply<false>(bytes + o, L, fill_load<false>(bytes + o, words + i), mode);
#endif
}

// Header-only generate (no payload bytes read): the IPv4 header checksum
// (ip.cc:266-278) and/or the tx-offload partial that a NIC completes — the
// folded pseudo-header stored in the L4 field (udp.cc:188-189, tcp.hh:1688-1689,
// `~csum.get()` of the pseudo-header alone; TSO: length 0 for TCP).
// One thread per frame.
__global__ __launch_bounds__(kBlock) void fill_header_kernel(uint8_t* __restrict__ bytes, uint64_t bytes_len,
                                                             const uint64_t* __restrict__ off,
                                                             const uint32_t* __restrict__ len,
                                                             uint32_t* __restrict__ out2,
                                                             uint8_t* __restrict__ status, uint64_t n, uint32_t mode) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = off[i];
    const uint32_t L = len[i];
    uint32_t word = 0, st = 0;
    if (o > bytes_len || L > bytes_len - o) {
        st = SCCSUM_ST_RANGE;
    } else if (L < 20u) {
        st = SCCSUM_ST_MALFORMED;
    } else {
        uint8_t* p = bytes + o;
        uint32_t h[10];  // little-endian 16-bit words of the 20-byte header
#pragma unroll
        for (int k = 0; k < 10; ++k) h[k] = static_cast<uint32_t>(p[2 * k]) | (static_cast<uint32_t>(p[2 * k + 1]) << 8);
        const FrameDecode D = frame_decode(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16),
                                           h[6] | (h[7] << 16), h[8] | (h[9] << 16), L);
        const uint32_t proto = D.proto, l4_off = D.l4_off, l4_len = D.l4_len;
        st |= D.st;
        if (mode & SCCSUM_FILL_IP) {
            const uint32_t ipc =
                ~fold16(static_cast<uint64_t>(h[0]) + h[1] + h[2] + h[3] + h[4] + h[6] + h[7] + h[8] + h[9]) & 0xffffu;
            p[10] = static_cast<uint8_t>(ipc);
            p[11] = static_cast<uint8_t>(ipc >> 8);
            word |= ipc;
            st |= SCCSUM_ST_OK;
        }
        if (mode & SCCSUM_FILL_L4_PSEUDO) {
            const uint32_t fo = proto == 17u ? 6u : (proto == 6u ? 16u : 0u);
            if (fo != 0u && l4_len >= fo + 2u && (st & (SCCSUM_ST_MALFORMED | SCCSUM_ST_IPFRAG)) == 0u &&
                D.ihl >= 5u) {
                const uint32_t plen = ((mode & SCCSUM_FILL_TSO) && proto == 6u) ? 0u : l4_len;
                const uint32_t ps = fold16(static_cast<uint64_t>(h[6]) + h[7] + h[8] + h[9] + (proto << 8) +
                                           swap16(plen & 0xffffu));
                p[l4_off + fo] = static_cast<uint8_t>(ps);
                p[l4_off + fo + 1] = static_cast<uint8_t>(ps >> 8);
                word |= ps << 16;
                st |= SCCSUM_ST_L4_OK;
            }
        }
    }
    if (out2) out2[i] = word;
    if (status) status[i] = static_cast<uint8_t>(st);
}

// Plain stream-read of the same load width (16 B per lane, nontemporal): one
// load per lane per step, grid-stride in launch order.  This simple form is the
// fastest plain read measured (tools/dev/store_probe.hip: 226 us per 1.57 GB =
// 6.95 TB/s; an earlier 4-loads-per-step form with an XCD block remap ran
// 6.7 TB/s), so it is the measured ceiling bench.py reports.
__global__ __launch_bounds__(kBlock) void read_probe_kernel(const u32x4* __restrict__ src, uint64_t units,
                                                             uint64_t* __restrict__ sink) {
    uint64_t acc = 0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < units; i += stride) {
        const u32x4 a = __builtin_nontemporal_load(src + i);
        acc += static_cast<uint64_t>(a.x) + a.y + a.z + a.w;
    }
    const uint32_t f = wave_sum(fold16(acc));
    if ((threadIdx.x & (kWave - 1)) == 0) {
        atomicAdd(reinterpret_cast<unsigned long long*>(sink + blockIdx.x), static_cast<unsigned long long>(f));
    }
}

// ---------------------------------------------------------------- host side

// The device a launch runs on.  HIP runs a kernel on its stream's device, and
// the memory contract (sccsum.h) puts the data on the calling thread's current
// device, so the stream must belong to that device: hipStreamGetDevice for a
// real stream (the null stream is the current device's).  A stream of another
// device is SCCSUM_EINVAL — it would otherwise read another device's pointers
// with this device's counter slot and grid size (VERDICT r03 missing #3).
// Everything a launch sizes or takes per device (CU count, counter pool)
// comes from the device returned here, not from a second hipGetDevice.
int launch_device(hipStream_t s, int* dev) {
    int cur = -1, sd = -1;  // cur stays -1 only when hipGetDevice itself failed
    const hipError_t e = host_launch::stream_devices(s, &cur, &sd);
    if (cur >= kMaxDevices) return SCCSUM_ENODEV;  // (decided before the stream is asked)
    if (e != hipSuccess) return static_cast<int>(e);
    if (cur < 0) return SCCSUM_ENODEV;
    if (sd != cur) return SCCSUM_EINVAL;
    *dev = cur;
    return SCCSUM_OK;
}

// An entry point's stream as HIP's type and the device its launches run on
// (launch_device); rc != SCCSUM_OK refuses the call.
struct LaunchTarget {
    hipStream_t s;
    int dev = 0;
    int rc;
    explicit LaunchTarget(void* stream) : s(static_cast<hipStream_t>(stream)), rc(launch_device(s, &dev)) {}
};

using host_launch::launch_kernel;
using host_launch::misaligned;

// Blocks of kBlock threads for one thread per item.
unsigned blocks_for(uint64_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); }

std::atomic<int> g_cu_count[kMaxDevices];

int cu_count(int dev) {
    if (dev < 0 || dev >= kMaxDevices) return 256;
    int c = g_cu_count[dev].load(std::memory_order_relaxed);
    if (c > 0) return c;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    g_cu_count[dev].store(c, std::memory_order_relaxed);
    return c;
}

int current_cu_count() {
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess ? cu_count(dev) : 256;
}

// Default tile target: about 48 KiB of packets per tile (32 x 1500 B frames,
// one 64 KiB segment; short packets stay at the 64-packet cap).  Measured
// against the plain 64-packet cap on every bench config (profiles/
// r02_ab_bench_tiles.log: cfg 2 +1.3-1.9 %, fill +1.7 %, cfg 4 +2.6 %, cfg 3
// unchanged): a launch's drain shrinks with the tile.  The packet count is
// what matters, and 32 is a sweet spot for 1500 B frames — 24-30 and 34-43
// packets per tile run slower than 64 (profiles/r02_ab_tiles2.log).
constexpr int kTileBytes = 49152;

// Tail split: the launch's last whole tiles (kTailQuarters / 4 per wave of the
// grid) are cut into kTailSplit sub-tiles each.  When the dequeue runs dry
// every wave is part-way through a tile and the launch ends with its slowest;
// short tiles at the end shorten that drain.
// A/B (profiles/r02_ab_tail.log): no gain on 1500 B frames (split 2-4: -0.3 %
// to -0.5 %), a loss on Zipf frames (split 4: +1.5 %, 8: +6.5 % time), so off.
constexpr int kTailSplit = 1;
constexpr int kTailQuarters = 4;

// Result stores nontemporal by default: the per-tile out2 / status stores mix
// into the read stream, and an nt (or sc1) store leaves less in the way than a
// plain one (profiles/r02_ab_outpol.log: 2 M frames 464.8 -> 460.2 us, Zipf
// frames 237.4 -> 235.5 us; sc1 / sc0 sc1 the same, sc0 no gain).
constexpr int kOutPolicy = 1;

// Run extents start on a 128-byte L2 line (8 units): a wave's 1 KiB load rows
// then cover 8 whole lines instead of 9 partial ones when a tile starts
// mid-line (odd offsets, 65 535 B segments).  Same-box A/B
// (profiles/r02_ab_run_align.log): Zipf frames 237.9 -> 234.2 us, 65 535 B
// spans 168.8 -> 166.7 us, 1500 B frames and 64 KiB spans -0.4-0.5 %; 64 B
// (4 units) lands in between.
constexpr int kRunAlign = 8;
// In-place fills (FILL_L4 / FILL_ICMP_ECHO) of at most this many frames store
// their fields from the generate tiles (kFlagFillNow) instead of a second pass.
// One pass wins up to 512 Ki frames on rotated batches (launch 171.7 against
// 181.3 us, engine 158.5 against 191.0) and loses at 1 Mi (launch 355 against
// 330 us, engine 341.7 against 330), where the stores inside the read stream
// cost more than the store pass (profiles/r05_fill_one_pass.log)
constexpr uint32_t kFillSingleMax = 524288;
// Single-batch launches of at most this many packets run the row kernel (launch)
constexpr uint64_t kSmallRowsMax = 65536;
static_assert(kRowQueues >= kMaxQueues, "a multi launch's batches fit the row kernel's table");

// Diagnostic knobs (include/sccsum_diag.h): per host thread, so one shard's
// A/B settings never leak into another thread's launches.
struct Knobs {
    int variant = 0;                 // 0 = default; 1 = simple kernel; 14-16 = flat-kernel forms
    int blocks_per_cu = kBlocksPerCU;  // grid cap in workgroups per CU
    int group_units = 0;             // simple kernel: U override (0 = by max_len)
    int tile_packets = kWave;        // flat kernel: max packets per tile
    int dynamic = 1;                 // flat kernel: dequeue tiles (1) or static round robin (0)
    int tile_bytes = kTileBytes;     // flat kernel: target bytes per tile (0 = packets cap only)
    int tail_split = kTailSplit;     // flat kernel: sub-tiles per tail tile (1, 2, 4 or 8; 1 = no split)
    int tail_quarters = kTailQuarters;  // flat kernel: tail = tail_quarters / 4 whole tiles per wave of the grid
    int out_policy = kOutPolicy;     // flat kernel: cache policy of the result stores (tile_store)
    int short_chunks = 1;            // flat kernel (no chunk in flight): a run's last chunk covers only its rows
    int run_align = kRunAlign;       // flat kernel: run extents start on 1 / 4 / 8-unit (16 / 64 / 128 B) boundaries
    int engine_wt = 1;               // engine: results written through (1) or stored as a launch stores them (0)
    int engine_idle_ms = 0;          // engine: overrides the engine's idle limit (ms) for runs this thread starts
    uint32_t fill_single_max = kFillSingleMax;  // in-place fills of at most this many frames run in one pass
    int engine_sync_every = -1;      // engine: every k-th step waits for the step before it (0 = never,
                                     // -1 = every kEngineSyncEvery steps of >= 2 tiles per wave)
};
thread_local Knobs t_knobs;

unsigned grid_for(uint64_t n, int dev) {
    const uint64_t cap = static_cast<uint64_t>(cu_count(dev)) * t_knobs.blocks_per_cu;
    uint64_t want = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    if (want > cap) want = cap;
    want = (want + 7) & ~uint64_t(7);  // multiple of 8 for the XCD mapping
    return static_cast<unsigned>(want);
}

// Tile-head counters for the flat kernel's dequeue: a pool of kSlots slots
// per device, each kGroups counters on their own 256-byte lines plus one
// completion counter, allocated and zeroed once, in sccsum_init.  Slots
// follow LAUNCHES, not streams: a launch takes a slot that no unfinished
// launch holds.  The kernel leaves the counters zeroed (the last dequeue of
// each group resets its counter) and, once all kGroups groups have reset,
// stores the launch's ticket into the slot's word of a pinned, host-coherent
// array; the host hands the slot out again only when that word equals the
// ticket it issued last.  So any number of streams and host threads may
// launch, and streams may be created and destroyed at any time (a destroyed
// stream's address reused by a new one shares nothing), with no allocation,
// no memset and no synchronisation on the launch path (VERDICT
// r02 weak #5).  A launch that finds no free slot among the next few of the
// ring, a launch being captured into a graph (a replay may run anywhere, any
// time), or one on a device nobody initialised uses the static tile order
// instead: the same results without the dynamic load balance.
constexpr uint32_t kSlots = 2048;
constexpr uint32_t kSlotProbe = 16;  // ring entries a launch checks before it falls back to the static order
constexpr uint32_t kSlotWords = (kGroups + 1) * kHeadStride;  // + the completion counter

struct DevicePool {
    std::mutex mu;
    std::atomic<uint32_t*> heads{nullptr};  // device: kSlots * kSlotWords words
    uint32_t* done = nullptr;               // pinned, host-coherent: ticket of each slot's last completed launch
    uint32_t* done_dev = nullptr;           // the same words as the device addresses them
    uint32_t issued[kSlots] = {};           // ticket of each slot's last launch (host)
    uint32_t cursor = 0;                    // next slot to try (ring order = launch order)
};
DevicePool g_pools[kMaxDevices];

int ensure_heads(int dev) {
    if (dev < 0 || dev >= kMaxDevices) return SCCSUM_ENODEV;
    DevicePool& P = g_pools[dev];
    std::lock_guard<std::mutex> g(P.mu);
    if (P.heads.load(std::memory_order_acquire) != nullptr) return SCCSUM_OK;
    void* m = nullptr;
    void* h = nullptr;
    void* hd = nullptr;
    const size_t bytes = size_t(kSlots) * kSlotWords * sizeof(uint32_t);
    hipError_t e = hipMalloc(&m, bytes);
    if (e == hipSuccess) e = hipMemset(m, 0, bytes);
    if (e == hipSuccess) {
        e = hipHostMalloc(&h, kSlots * sizeof(uint32_t),
                          hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable);
    }
    if (e == hipSuccess) e = hipHostGetDevicePointer(&hd, h, 0);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (m) (void)hipFree(m);
        if (h) (void)hipHostFree(h);
        return static_cast<int>(e);
    }
    P.done = static_cast<uint32_t*>(h);
    for (uint32_t i = 0; i < kSlots; ++i) __atomic_store_n(&P.done[i], 0u, __ATOMIC_RELAXED);
    P.done_dev = static_cast<uint32_t*>(hd);
    P.heads.store(static_cast<uint32_t*>(m), std::memory_order_release);
    return SCCSUM_OK;
}

// A launch's hold on a slot: the counters, where the kernel reports
// completion and the ticket it reports.  heads == nullptr: static tile order.
struct HeadSlot {
    uint32_t* heads = nullptr;
    uint32_t* done = nullptr;
    uint32_t ticket = 0;
    int dev = -1;
    uint32_t idx = 0;
};

HeadSlot acquire_heads(hipStream_t s, int dev) {
    HeadSlot H;
    if (dev < 0 || dev >= kMaxDevices) return H;
    DevicePool& P = g_pools[dev];
    uint32_t* const heads = P.heads.load(std::memory_order_acquire);
    if (heads == nullptr) return H;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return H;
    std::lock_guard<std::mutex> g(P.mu);
    for (uint32_t k = 0; k < kSlotProbe; ++k) {
        const uint32_t i = (P.cursor + k) % kSlots;
        if (__atomic_load_n(&P.done[i], __ATOMIC_ACQUIRE) != P.issued[i]) continue;  // still running
        H.ticket = ++P.issued[i];
        H.heads = heads + size_t(kSlotWords) * i;
        H.done = P.done_dev + i;
        H.dev = dev;
        H.idx = i;
        P.cursor = (i + 1) % kSlots;
        return H;
    }
    return H;
}

// A launch that did not start never reports: hand its slot back.
void release_unlaunched(const HeadSlot& H) {
    if (H.heads == nullptr) return;
    DevicePool& P = g_pools[H.dev];
    std::lock_guard<std::mutex> g(P.mu);
    __atomic_store_n(&P.done[H.idx], H.ticket, __ATOMIC_RELEASE);
}

int units_class(uint32_t max_len) {
    const int forced = t_knobs.group_units;
    if (forced) return forced;
    if (max_len == 0) return 4;
    const uint64_t units = (static_cast<uint64_t>(max_len) + 30) / 16;  // worst-case head of 15
    if (units <= 64) return 1;
    if (units <= 128) return 2;
    if (units <= 256) return 4;
    return 8;
}

// Flat-kernel launch: the grid is what the chip holds at once (the kernel's
// occupancy, from its VGPR and LDS use, capped by the blocks-per-CU knob), so
// every wave's static first tile starts at launch; tiles hold B packets (one
// per lane, B <= 64, about tile_bytes of packets when that knob is set),
// numbered across the queue set.
using FlatKernel = void (*)(const Queues, uint32_t, uint32_t*, uint32_t*, uint32_t, uint32_t, const RssParams);

// Resident 256-thread blocks per CU of a kernel (from its VGPR and LDS use),
// cached per kernel.
int kernel_occupancy(const void* k) {
    constexpr int kSlots = 32;
    static std::atomic<const void*> keys[kSlots];
    static std::atomic<int> vals[kSlots];
    for (int i = 0; i < kSlots; ++i) {
        if (keys[i].load(std::memory_order_acquire) == k) return vals[i].load(std::memory_order_relaxed);
    }
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, kBlock, 0) != hipSuccess || nb <= 0) nb = 1;
    for (int i = 0; i < kSlots; ++i) {
        const void* expect = nullptr;
        if (keys[i].load(std::memory_order_relaxed) == nullptr) {
            vals[i].store(nb, std::memory_order_relaxed);
            if (keys[i].compare_exchange_strong(expect, k, std::memory_order_release)) break;
        }
    }
    return nb;
}

// Blocks of a kernel the device holds at once: its occupancy, capped by the
// blocks-per-CU knob, on every CU.  Each launch rounds this its own way.
template <class Kern>
uint64_t resident_blocks(Kern kern, int dev) {
    const int occ = kernel_occupancy(reinterpret_cast<const void*>(kern));
    return static_cast<uint64_t>(cu_count(dev)) * (occ < t_knobs.blocks_per_cu ? occ : t_knobs.blocks_per_cu);
}

// Packets per tile of a flat launch or of an engine's summing step: about
// tile_bytes of packets, at most tile_packets (<= 64, one per lane), and no
// fewer tiles than there are wave slots (the caller's: a launch's grid cap, a
// running engine's grid).  pbytes is packet_bytes() of the batches, so the
// mean packet is floor(min(bytes, n * max_len) / n), which equals
// min(floor(bytes / n), max_len): max_len caps the mean either way round.
uint64_t packets_per_tile(uint64_t n_total, uint64_t pbytes, uint64_t slots, const Knobs& K) {
    uint64_t bmax = static_cast<uint64_t>(K.tile_packets);
    const uint64_t tb = static_cast<uint64_t>(K.tile_bytes);
    if (tb && n_total) {
        const uint64_t mean = pbytes / n_total ? pbytes / n_total : 1;
        const uint64_t bb = tb / mean ? tb / mean : 1;
        bmax = bb < bmax ? bb : bmax;
    }
    const uint64_t B = slots ? (n_total + slots - 1) / slots : 1;
    return B < 1 ? 1 : (B > bmax ? bmax : B);
}

// The knobs every summing kernel takes as flag bits.
uint32_t knob_flags(const Knobs& K) {
    return static_cast<uint32_t>(K.out_policy) << kOutPolicyShift | (K.short_chunks ? 0u : kFlagFullChunks) |
           static_cast<uint32_t>(K.run_align == 8 ? 2 : (K.run_align == 4 ? 1 : 0)) << kRunAlignShift;
}

// Q holds the queues (nq >= 1); tile0 is filled here from the tile size.
// `dev` is the stream's device (launch_device).
hipError_t launch_flat(FlatKernel kern, hipStream_t s, int dev, Queues& Q, uint64_t n_total, uint64_t bytes_total,
                       uint32_t flags, const RssParams& rss) {
    const Knobs& K = t_knobs;
    const uint64_t cap = resident_blocks(kern, dev);
    const uint64_t slots = cap * kWavesPerBlock;
    const uint64_t B = packets_per_tile(n_total, bytes_total, slots, K);
    Q.tile0[0] = 0;
    for (uint32_t q = 0; q < Q.nq; ++q) Q.tile0[q + 1] = Q.tile0[q] + (Q.n[q] + B - 1) / B;
    const uint64_t whole = Q.tile0[Q.nq];
    // tail split (sub-tiles of at least one packet, a power of two per tile)
    uint32_t lg = 0;
    while ((2u << lg) <= static_cast<uint32_t>(K.tail_split) && (2ull << lg) <= B) ++lg;
    const uint64_t tail = lg ? static_cast<uint64_t>(K.tail_quarters) * slots / 4 : 0;
    Q.tsplit = whole > tail ? whole - tail : 0;
    Q.sub_log2 = lg;
    Q.bsub = static_cast<uint32_t>((B + (1u << lg) - 1) >> lg);
    const uint64_t tiles = Q.tsplit + ((whole - Q.tsplit) << lg);
    uint64_t blocks = (tiles + kWavesPerBlock - 1) / kWavesPerBlock;
    blocks = blocks < cap ? blocks : cap;
    blocks = (blocks + 15) & ~uint64_t(15);  // multiple of 16: XCD mapping, waves divide into kGroups
    // A launch of at most one tile per wave has nothing to balance: its tiles
    // are dealt round robin, with no counter slot and no claim round trip
    // (small launches 0.5-0.9 us faster, profiles/r05_fill_one_pass.log)
    const bool dyn = K.dynamic && tiles > blocks * kWavesPerBlock;
    const HeadSlot H = dyn ? acquire_heads(s, dev) : HeadSlot{};
    // the launch's own error decides whether the slot goes back: a kernel that
    // did not start never reports completion
    const hipError_t e = launch_kernel(kern, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s, Q,
                                       static_cast<uint32_t>(B), H.heads, H.done, H.ticket, flags | knob_flags(K), rss);
    if (e != hipSuccess) release_unlaunched(H);
    return e;
}

template <bool IPV4>
hipError_t launch_simple(int uc, hipStream_t s, int dev, const uint8_t* b, uint64_t bytes_len, const uint64_t* d_off,
                         const uint32_t* d_len, const uint32_t* d_seed, uint16_t* d_out, uint8_t* d_status,
                         uint64_t n, uint32_t flags) {
    const dim3 g(grid_for(n, dev));
    auto go = [&](auto kern) {
        return launch_kernel(kern, g, dim3(kBlock), 0, s, b, bytes_len, d_off, d_len, d_seed, d_out, d_status, n,
                             flags);
    };
    switch (uc) {
        case 1: return go(csum_kernel<1, IPV4>);
        case 2: return go(csum_kernel<2, IPV4>);
        case 4: return go(csum_kernel<4, IPV4>);
        default: return go(csum_kernel<8, IPV4>);
    }
}

template <bool IPV4, bool MQ = false, bool FILL = false>
hipError_t launch_rows(uint32_t max_len, hipStream_t s, int dev, const uint8_t* b, uint64_t bytes_len,
                       const uint64_t* d_off, const uint32_t* d_len, const uint32_t* d_seed, uint16_t* d_out,
                       uint8_t* d_status, uint64_t n, uint32_t flags, const RowQueues& rq = RowQueues{}) {
    const uint64_t units = max_len ? (static_cast<uint64_t>(max_len) + 30u) / 16u : 128u;  // worst-case head of 15
    // the grid is what the chip holds at once (a grid-stride kernel: blocks
    // that only start when others end would make the tail)
    auto go = [&](auto kern) {
        const uint64_t cap = resident_blocks(kern, dev);
#ifdef SCCSUM_AB_ROWS_TILE64
        uint64_t blocks = ((n + 63u) / 64u + kWavesPerBlock - 1) / kWavesPerBlock;  // A/B: 64-packet tiles
#else
        // waves for every four packets (one row step each) up to what the chip
        // holds: a launch too small to fill the chip splits its packets evenly
        // into short tiles (the kernel's last-round rule) instead of giving
        // each of n / 64 waves 16 row steps one after another
        uint64_t blocks = ((n + 3u) / 4u + kWavesPerBlock - 1) / kWavesPerBlock;
#endif
        blocks = blocks < cap ? blocks : cap;
        blocks = (blocks + 7u) & ~uint64_t(7);  // multiple of 8 for the XCD mapping
        return launch_kernel(kern, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s, b, bytes_len, d_off, d_len,
                             d_seed, d_out, d_status, n, flags, rq);
    };
    if (units <= 32) return go(csum_row_kernel<2, IPV4, MQ, FILL>);
    if (units <= 64) return go(csum_row_kernel<4, IPV4, MQ, FILL>);
    if (units <= 96) return go(csum_row_kernel<6, IPV4, MQ, FILL>);  // 1500 B frames: 95 units
    return go(csum_row_kernel<8, IPV4, MQ, FILL>);
}

// Flat-kernel forms: 14 / 15 = U 8 (15: the next chunk in flight), 16 = U 16.
// (U 2 / 4 forms and rolling rows lost their A/Bs in rounds 1-2 and were
// removed: profiles/r01_ab_variants.log, r02_ab_roll.log.)  Frames may fill
// in place; spans never do.
template <bool IPV4>
hipError_t launch_flat_variant(int variant, hipStream_t s, int dev, Queues& Q, uint64_t n_total, uint64_t bytes_total,
                               uint32_t flags, const RssParams& rss) {
    auto go = [&](auto kern) { return launch_flat(kern, s, dev, Q, n_total, bytes_total, flags, rss); };
    constexpr bool F = IPV4;
    const bool fill = IPV4 && (flags & kFillFlags);
    // the chunk-in-flight form's late claim pays for packets of 1 KiB or more in
    // launches of several tiles per wave (flat_body, PLATE): one tile per wave
    // (2 x 32 768 frames) ran 3.5 % slower with it, the launch's last atomic
    // then waited on at the wave's end
    const bool plate = n_total != 0 && bytes_total / n_total >= 1024u && bytes_total >= (uint64_t(256) << 20);
    switch (variant) {
        case 14: return fill ? go(csum_flat_kernel<8, IPV4, F, false>) : go(csum_flat_kernel<8, IPV4, false, false>);
        case 15:
            if (fill) return plate ? go(csum_flat_kernel<8, IPV4, F, true, true>) : go(csum_flat_kernel<8, IPV4, F, true>);
            return plate ? go(csum_flat_kernel<8, IPV4, false, true, true>) : go(csum_flat_kernel<8, IPV4, false, true>);
        default: return fill ? go(csum_flat_kernel<16, IPV4, F, false>) : go(csum_flat_kernel<16, IPV4, false, false>);
    }
}

// Host-side Toeplitz windows: w[j] = the 32 key bits starting at bit j (MSB
// first), bits past key_len zero — what toeplitz.hh:84-94 holds in `v` when it
// reaches data bit j.
RssParams make_rss(const uint8_t* key, uint32_t key_len, uint32_t mode, uint32_t* d_hash) {
    RssParams P{};
    P.hash = d_hash;
    P.mode = mode;
    auto bit = [&](uint32_t k) -> uint32_t { return k < 8u * key_len ? (key[k >> 3] >> (7u - (k & 7u))) & 1u : 0u; };
    for (uint32_t j = 0; j < 96; ++j) {
        uint32_t w = 0;
        for (uint32_t t = 0; t < 32; ++t) w |= bit(j + t) << (31u - t);
        P.w[j] = w;
    }
    return P;
}

const RssParams kNoRss{};

// One batch's arguments, checked as every entry point checks them.
template <bool IPV4>
bool batch_ok(const void* d_bytes, const uint64_t* d_off, const uint32_t* d_len, const uint32_t* d_seed,
              const void* d_out, const uint8_t* d_status, uint32_t flags) {
    // frames: a verify-only launch may pass the status array alone (the
    // reference's verify only tests get() != 0, ip.cc:121-127, tcp.hh:876-883)
    const bool out_optional = (flags & kFillFlags) || (IPV4 && d_status != nullptr);
    if (!d_bytes || !d_off || !d_len || (!d_out && !out_optional)) return false;
    return !(misaligned(d_bytes, 16) || misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_seed, 4) ||
             misaligned(d_out, IPV4 ? 4 : 2));
}

// The next queue of a launch's table (Queues or RowQueues) from a batch; each
// table keeps the packet counts its own way.
void put_count(Queues& Q, uint32_t q, uint64_t n) { Q.n[q] = n; }
void put_count(RowQueues& Q, uint32_t q, uint64_t n) { Q.first[q + 1] = Q.first[q] + n; }
template <class Table>
void add_queue(Table& Q, const sccsum_batch& x) {
    const uint32_t q = Q.nq++;
    Q.bytes[q] = static_cast<const uint8_t*>(x.d_bytes);
    Q.bytes_len[q] = x.bytes_len;
    Q.off[q] = x.d_off;
    Q.len[q] = x.d_len;
    Q.seed[q] = x.d_seed;
    Q.out[q] = static_cast<uint16_t*>(x.d_out);
    Q.status[q] = x.d_status;
    put_count(Q, q, x.n);
}

// default: the flat kernel, all loads nontemporal — 16 units per lane per
// chunk for big launches (>= 512 Ki packets and 256 MiB), else 8 units with
// the next chunk in flight: the 16-unit form runs 2 waves per SIMD, too few
// tiles per wave on smaller launches (DESIGN.md §5.1 has the A/B)
//
// Sparse layouts go to the row kernel (one packet per 16-lane row): when the
// buffer holds at least max_len + 64 bytes per packet, the mean gap between
// packets is over 4 units, each packet is its own run and a flat-kernel wave
// waits out one round trip per packet, one after another.  1500 B frames in
// 2304 B mbuf slots (data at +256), per 1 M frames: flat 537 us (920 without
// short chunks), one wave per packet 359-368 us, one row per packet 253-259 us
// (profiles/r02_ab_slots.log, r02_ab_rows.log).
// The bytes a launch's packets can span: bytes_len, capped by n * max_len when
// the caller gives max_len.  A batch that is a slice of a larger buffer (a
// shard's rx ring handed over a burst at a time; offsets into the whole ring)
// has a bytes_len far above its packets' bytes, and sizing tiles or picking
// the form from it gave such a launch tiles of one or two packets: a
// 16 384-frame fill on a slice of a 393 MB ring took 26.0 us a launch with
// 2-frame tiles, 16.9 with 8-frame ones (profiles/r05_engine_small_steps_final.log).
uint64_t packet_bytes(uint64_t n_total, uint64_t bytes_total, uint32_t max_len) {
    if (max_len == 0) return bytes_total;
    const uint64_t cap = n_total * static_cast<uint64_t>(max_len);
    return cap < bytes_total ? cap : bytes_total;
}

int pick_variant(uint64_t n_total, uint64_t bytes_total, uint32_t flags, uint32_t max_len) {
    int variant = t_knobs.variant;
    const uint64_t pb = packet_bytes(n_total, bytes_total, max_len);
    const int dflt = (n_total >= (512u << 10) && pb >= (256ull << 20)) ? 16 : 15;
    const bool fill = (flags & kFillFlags) != 0;
    const bool sparse = max_len != 0 && n_total != 0 && bytes_total / n_total >= uint64_t(max_len) + 64u;
    if (variant == 0 && sparse && !fill) return 2;
    if (variant == 0 || ((variant == 1 || variant == 2) && fill)) variant = dflt;  // in-place write-back: flat only
    return variant;
}

template <bool IPV4>
int launch(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
           const uint32_t* d_seed, uint16_t* d_out, uint8_t* d_status, uint64_t n, uint32_t max_len,
           void* stream, uint32_t flags = 0, const RssParams& rss = kNoRss) {
    if (n == 0) return SCCSUM_OK;
    if (!batch_ok<IPV4>(d_bytes, d_off, d_len, d_seed, d_out, d_status, flags)) return SCCSUM_EINVAL;
    const LaunchTarget T(stream);
    if (T.rc != SCCSUM_OK) return T.rc;
    int variant = pick_variant(n, bytes_len, flags, max_len);
    // a small single-batch launch runs the row kernel whatever the layout:
    // four packets per wave in one row step reach the results sooner than the
    // flat kernel's plan, scan and pick-up (dense 1500 B batches, eager: 32
    // packets 4.2 against 6.4 us, 1 024 4.5 against 6.9, 16 384 8.4 against
    // 11.3, 65 536 22.5 against 23.8; level at 262 144, 10 % slower at 1 M;
    // profiles/r05_ab_rows_small.log).  In-place fills (sccsum_ipv4_fill picks
    // its own kernel) and fused RSS stay on the flat kernel here; small multi
    // launches take the row kernel's several-batch form (launch_multi).
    if (t_knobs.variant == 0 && variant != 2 && n <= kSmallRowsMax && !(flags & kFillFlags) && rss.hash == nullptr) {
        variant = 2;
    }
    const uint8_t* b = static_cast<const uint8_t*>(d_bytes);
    if (variant == 1 || variant == 2) {
        hipError_t e = variant == 1
                           ? launch_simple<IPV4>(units_class(max_len), T.s, T.dev, b, bytes_len, d_off, d_len, d_seed,
                                                 d_out, d_status, n, flags)
                           : launch_rows<IPV4>(max_len, T.s, T.dev, b, bytes_len, d_off, d_len, d_seed, d_out, d_status,
                                               n, flags);
        if (e == hipSuccess && IPV4 && rss.hash != nullptr) {  // RSS is fused only in the flat kernel
            e = launch_kernel(rss_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, T.s, b, bytes_len, d_off, d_len,
                              nullptr, n, rss);
        }
        return static_cast<int>(e);
    } else {
        Queues Q{};
        add_queue(Q, sccsum_batch{d_bytes, bytes_len, d_off, d_len, d_seed, d_out, d_status, n});
        return static_cast<int>(
            launch_flat_variant<IPV4>(variant, T.s, T.dev, Q, n, packet_bytes(n, bytes_len, max_len), flags, rss));
    }
}

// Several independent batches in one flat-kernel launch (sccsum_*_multi).
template <bool IPV4>
int launch_multi(const sccsum_batch* batches, uint32_t nbatch, uint32_t max_len, void* stream) {
    if (nbatch > kMaxQueues || (nbatch && !batches)) return SCCSUM_EINVAL;
    uint64_t n_total = 0, bytes_total = 0;
    for (uint32_t i = 0; i < nbatch; ++i) {
        const sccsum_batch& x = batches[i];
        if (x.n && !batch_ok<IPV4>(x.d_bytes, x.d_off, x.d_len, IPV4 ? nullptr : x.d_seed, x.d_out, x.d_status, 0)) {
            return SCCSUM_EINVAL;
        }
        if (IPV4 && x.d_seed) return SCCSUM_EINVAL;  // frames derive their pseudo-header in-kernel
        n_total += x.n;
        bytes_total += x.n ? x.bytes_len : 0;
    }
    if (n_total == 0) return SCCSUM_OK;
    const LaunchTarget T(stream);
    if (T.rc != SCCSUM_OK) return T.rc;
    const int variant = pick_variant(n_total, bytes_total, 0, max_len);
    // a small multi launch runs the row kernel over all its batches at once
    // (as a small single-batch launch does, launch(): 16 x 32 frames 6.3 ->
    // profiles/r05_ab_rows_small.log)
    if (t_knobs.variant == 0 && n_total <= kSmallRowsMax) {
        RowQueues rq{};
        for (uint32_t i = 0; i < nbatch; ++i) {
            if (batches[i].n) add_queue(rq, batches[i]);
        }
        return static_cast<int>(launch_rows<IPV4, true>(max_len, T.s, T.dev, nullptr, 0, nullptr, nullptr, nullptr,
                                                        nullptr, nullptr, n_total, 0, rq));
    }
    if (variant == 1 || variant == 2) {  // the per-packet kernels take one batch per launch
        for (uint32_t i = 0; i < nbatch; ++i) {
            const sccsum_batch& x = batches[i];
            if (!x.n) continue;
            const auto* b = static_cast<const uint8_t*>(x.d_bytes);
            auto* o = static_cast<uint16_t*>(x.d_out);
            const hipError_t e =
                variant == 1 ? launch_simple<IPV4>(units_class(max_len), T.s, T.dev, b, x.bytes_len, x.d_off,
                                                   x.d_len, x.d_seed, o, x.d_status, x.n, 0)
                             : launch_rows<IPV4>(max_len, T.s, T.dev, b, x.bytes_len, x.d_off, x.d_len, x.d_seed,
                                                 o, x.d_status, x.n, 0);
            if (e != hipSuccess) return static_cast<int>(e);
        }
        return SCCSUM_OK;
    }
    Queues Q{};
    for (uint32_t i = 0; i < nbatch; ++i) {
        if (batches[i].n) add_queue(Q, batches[i]);  // (a frames batch's d_seed is NULL: checked above)
    }
    return static_cast<int>(launch_flat_variant<IPV4>(variant, T.s, T.dev, Q, n_total,
                                                      packet_bytes(n_total, bytes_total, max_len), 0, kNoRss));
}

// ---- gather: fragments from device-readable memory (HBM, or pinned host
// memory read over PCIe) into one device buffer.  The burst queue's zero-copy
// submit (burst.cc) uses it so that no host thread touches packet bytes.
// One wave per fragment, grid-stride; interior 16-byte blocks of the
// destination move as one (possibly unaligned) 16-byte load + one aligned
// store, the two edge blocks byte by byte (neighbouring fragments are written
// by other waves at the same time).
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));

__global__ __launch_bounds__(kBlock) void gather_kernel(const sccsum_gather_desc* __restrict__ desc, uint64_t n,
                                                        uint8_t* __restrict__ dst) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nw = static_cast<uint64_t>(gridDim.x) * (kBlock / 64);
    for (uint64_t w = (static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x) >> 6; w < n; w += nw) {
        const sccsum_gather_desc d = desc[w];
        if (!d.src) continue;  // already in the batch (a copied packet of a mixed burst)
        const uint8_t* src = static_cast<const uint8_t*>(d.src);
        uint8_t* o = dst + d.dst_off;
        const uintptr_t a = reinterpret_cast<uintptr_t>(o), e = a + d.len;
        for (uintptr_t blk = (a & ~uintptr_t(15)) + 16u * lane; blk < e; blk += 1024u) {
            if (blk >= a && blk + 16u <= e) {
                *reinterpret_cast<u32x4*>(blk) = *reinterpret_cast<const u32x4u*>(src + (blk - a));
            } else {
                for (uint32_t k = 0; k < 16u; ++k) {
                    const uintptr_t p = blk + k;
                    if (p >= a && p < e) *reinterpret_cast<uint8_t*>(p) = src[p - a];
                }
            }
        }
    }
}

// ---- fragment-list kernel: packets given as descriptor lists over
// device-readable memory (HBM, or pinned / registered host memory read over
// PCIe), summed where they lie — the bytes are read once, straight into the
// sum, with no gather into a contiguous batch first (checksummer::sum(const
// packet&), ip_checksum.cc:64-68, over fragments anywhere).  Packet p has
// fragments desc[first[p] .. first[p+1]); fragment j holds packet bytes
// [dst_off_j - off[p], + len_j) — they must tile [0, len[p]) in order — and
// lies at src_j, or at stage + dst_off_j when src_j is NULL (bytes already in
// the batch).  One wave per packet at a time (grid-stride; a wave loads the
// metadata of its next 64 packets one per lane first), U 16-byte units per
// lane in flight; a one-fragment packet takes the contiguous-span path.  A fragment's bytes are summed at their address parity and the
// fragment's folded sum byte-swapped when its address and its packet offset
// differ in parity (the odd carry of the reference's fragment loop).
//
// FILL (frames only; flags = the SCCSUM_FILL_* mode): generate and store in
// place, the tx form (tcp.hh:1691-1694, udp.cc:184-195, ip.cc:266-278,
// ip.cc:464-474 over a fragment list).  Same validation and header decode;
// every sum leaves its own field out (the IP sum bytes 10-11, the L4 sum the
// TCP / UDP field, an echo request's sum its type, code and checksum bytes:
// the bytes are masked while summing, so an all-zero message keeps the
// reference's zero), so what the fields held does not matter.  The payload is
// read only when a sum over it is stored (FILL_L4 on a TCP / UDP frame that
// gets its field, FILL_ICMP_ECHO on an echo request).  The wave then stores
// at most six bytes itself, one per lane; each lane picks up its byte's
// address as the fragment loop passes over it (a field's two bytes may lie in
// different fragments: walking the descriptors again after the sum cost two
// more dependent round trips per packet); the skip rules are fill_apply's.
// Every stored value depends on the wave's loads, the stored bytes are left
// out of the wave's own sums, and no wave waits for another.  One-fragment
// packets take the general path here (one more round trip than
// span_packet's; DESIGN.md "Fill on fragment lists").
template <int U, bool IPV4, bool FILL = false>
__global__ __launch_bounds__(kBlock) void csum_desc_kernel(
    const sccsum_gather_desc* __restrict__ desc, const uint32_t* __restrict__ first,
    const uint64_t* __restrict__ off, const uint32_t* __restrict__ len, const uint32_t* __restrict__ seed,
    const uint8_t* __restrict__ stage, uint16_t* __restrict__ out, uint8_t* __restrict__ status, uint64_t n,
    uint32_t flags) {
    static_assert(!FILL || IPV4, "in-place generate is a frames mode");
    const bool raw = !IPV4 && (flags & kFlagRaw);
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kWavesPerBlock;
    auto frag_addr = [&](const sccsum_gather_desc& d) {
        return d.src ? reinterpret_cast<uintptr_t>(d.src) : reinterpret_cast<uintptr_t>(stage + d.dst_off);
    };

    auto rl32 = [](uint32_t v, uint32_t k) {
        return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(k)));
    };
    auto rl64 = [&](uint64_t v, uint32_t k) {
        return static_cast<uint64_t>(rl32(static_cast<uint32_t>(v), k)) |
               static_cast<uint64_t>(rl32(static_cast<uint32_t>(v >> 32), k)) << 32;
    };
    // A wave's packets are p0, p0 + stride, ...: their metadata and first
    // descriptors are loaded 64 at a time, one packet per lane (two round trips
    // for up to 64 packets — over PCIe when the arrays are pinned host memory),
    // then each packet costs one round trip for its bytes.
    const uint64_t p0 = static_cast<uint64_t>(xcd_block_id()) * kWavesPerBlock + wv;
    for (uint64_t base = p0; base < n; base += kWave * stride) {
        const uint64_t q = base + lane * stride;
        uint64_t m_off = 0, m_src = 0;
        uint32_t m_len = 0, m_f0 = 0, m_f1 = 0, m_dst = 0, m_dlen = 0;
        if (q < n) {
            m_off = off[q];
            m_len = len[q];
            m_f0 = first[q];
            m_f1 = desc ? first[q + 1] : m_f0;  // no descriptor array: no packet has fragments
        }
        if (q < n && m_f1 > m_f0) {
            const sccsum_gather_desc d = desc[m_f0];
            m_src = reinterpret_cast<uint64_t>(d.src);
            m_dst = d.dst_off;
            m_dlen = d.len;
        }
        const uint64_t left = (n - base + stride - 1) / stride;
        const uint32_t cnt = left < kWave ? static_cast<uint32_t>(left) : kWave;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint64_t p = base + k * stride;
            const uint64_t o = rl64(m_off, k);
            const uint32_t L = rl32(m_len, k);
            const uint32_t f0 = rl32(m_f0, k), f1 = rl32(m_f1, k);
            sccsum_gather_desc d0{};
            d0.src = reinterpret_cast<const void*>(rl64(m_src, k));
            d0.dst_off = rl32(m_dst, k);
            d0.len = rl32(m_dlen, k);
            // the fragments must tile the packet: [0, L) in order, no gaps
            bool bad = f1 < f0;
            if (f1 - f0 == 1) {
                bad = d0.dst_off != o || d0.len != L || (!d0.src && !stage);
            } else if (!bad) {
                uint64_t at = 0;
                for (uint32_t j = f0; j < f1 && !bad; ++j) {
                    const sccsum_gather_desc d = desc[j];
                    bad = static_cast<uint64_t>(d.dst_off) != o + at || (!d.src && !stage);
                    at += d.len;
                }
                bad = bad || at != L;
            }
            if (bad || (IPV4 && L < 20)) {
                if (lane == 0) {
                    if (IPV4) {
                        if (!FILL || out) reinterpret_cast<uint32_t*>(out)[p] = 0;
                    } else {
                        out[p] = 0;
                    }
                    if (status) status[p] = bad ? SCCSUM_ST_RANGE : SCCSUM_ST_MALFORMED;
                }
                continue;
            }

            // FILL: the address of packet byte `pos` (< L), from whichever fragment holds it
            [[maybe_unused]] auto locate = [&](uint32_t pos) -> uintptr_t {
                uint32_t at = 0;
                for (uint32_t j = f0; j < f1; ++j) {
                    const sccsum_gather_desc d = desc[j];
                    if (pos < at + d.len) return frag_addr(d) + (pos - at);
                    at += d.len;
                }
                return 0;
            };
            uint32_t S = 0, ipc = 0, pseudo = 0;
            uint8_t st = 0;
            // FILL: which fields this packet gets (wave-uniform) and the packet
            // bytes [xl, xh) its L4 sum leaves out
            [[maybe_unused]] bool put_l4 = false, echo = false;
            [[maybe_unused]] uint32_t l4_off = 0, l4_fo = 0, xl = 0, xh = 0;
            // FILL, per lane: the packet byte lane k < 6 stores, whether it does, and
            // that byte's address, picked up as the fragment loop passes over it
            [[maybe_unused]] uint32_t spos = 0;
            [[maybe_unused]] bool son = false;
            [[maybe_unused]] uintptr_t saddr = 0;
            if (!FILL && f1 - f0 <= 1) {
                // one fragment (or an empty packet): the contiguous-span path, header
                // and first units in one round trip
                const uint8_t* ptr = L ? reinterpret_cast<const uint8_t*>(frag_addr(d0)) : stage;
                const PacketSum R = span_packet<U, IPV4>(ptr, L, static_cast<int>(lane));
                S = R.S;
                ipc = R.ipc;
                pseudo = R.pseudo;
                st = R.st;
            } else {
                uint32_t rs = 0, re = L;
                if (IPV4) {
                    // header byte `lane` (lanes 0..19) from whichever fragment holds it
                    uint32_t hb = 0;
                    if (lane < 20u) {
                        uint32_t at = 0;
                        for (uint32_t j = f0; j < f1; ++j) {
                            const sccsum_gather_desc d = desc[j];
                            if (lane < at + d.len) {
                                hb = reinterpret_cast<const uint8_t*>(frag_addr(d))[lane - at];
                                break;
                            }
                            at += d.len;
                        }
                    }
                    uint32_t h[5];
    #pragma unroll
                    for (int k = 0; k < 5; ++k) {
                        h[k] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(hb), 4 * k)) |
                               static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(hb), 4 * k + 1)) << 8 |
                               static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(hb), 4 * k + 2)) << 16 |
                               static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(hb), 4 * k + 3)) << 24;
                    }
                    if constexpr (FILL) {
                        const FrameDecode D = frame_decode(h[0], h[1], h[2], h[3], h[4], L);
                        st = static_cast<uint8_t>(D.st);
                        l4_off = D.l4_off;
                        if (flags & SCCSUM_FILL_IP) {
                            ipc = ~fold16(static_cast<uint64_t>(h[0]) + h[1] + (h[2] & 0xffffu) + h[3] + h[4]) & 0xffffu;
                            st |= SCCSUM_ST_OK;
                        }
                        // as fill_apply: malformed, an IP fragment, or ihl < 5 -> no L4 write
                        const bool atomic = (D.st & (SCCSUM_ST_MALFORMED | SCCSUM_ST_IPFRAG)) == 0u && D.ihl >= 5u;
                        l4_fo = D.proto == 17u ? 6u : (D.proto == 6u ? 16u : 0u);
                        put_l4 = (flags & (SCCSUM_FILL_L4 | SCCSUM_FILL_L4_PSEUDO)) != 0u && l4_fo != 0u && atomic &&
                                 D.l4_len >= l4_fo + 2u;
                        if ((flags & SCCSUM_FILL_ICMP_ECHO) && D.proto == 1u && atomic && D.l4_len >= 8u) {
                            uint32_t type = 0;
                            if (lane == 0) type = *gld(reinterpret_cast<const uint8_t*>(locate(l4_off)));
                            echo = __builtin_amdgcn_readfirstlane(type) == 8u;  // echo_request (ip.cc:469)
                        }
                        if (flags & SCCSUM_FILL_L4_PSEUDO) {
                            // the partial a NIC completes: the folded pseudo-header (TSO: TCP length 0)
                            pseudo = ((flags & SCCSUM_FILL_TSO) && D.proto == 6u)
                                         ? fold16(static_cast<uint64_t>(h[3] & 0xffffu) + (h[3] >> 16) +
                                                  (h[4] & 0xffffu) + (h[4] >> 16) + (D.proto << 8))
                                         : D.pseudo;
                        } else {
                            pseudo = D.pseudo;  // 0 for ICMP
                        }
                        const bool sum = echo || (put_l4 && (flags & SCCSUM_FILL_L4));
                        rs = sum ? l4_off : 0u;
                        re = sum ? l4_off + D.l4_len : 0u;
                        xl = l4_off + (echo ? 0u : l4_fo);
                        xh = xl + (echo ? 4u : 2u);
                        // lanes 0-1 the IP field, 2-3 the L4 field, 4-5 an echo reply's type and code
                        if (lane < 2u) {
                            son = (flags & SCCSUM_FILL_IP) != 0u;
                            spos = 10u + lane;
                        } else if (lane < 4u) {
                            son = put_l4 || echo;
                            spos = l4_off + (echo ? 2u : l4_fo) + (lane - 2u);
                        } else if (lane < 6u) {
                            son = echo;
                            spos = l4_off + (lane - 4u);
                        }
                    } else {
                        const FrameHeader F = frame_header(h[0], h[1], h[2], h[3], h[4], L);
                        ipc = F.ipc;
                        st = F.st;
                        pseudo = F.pseudo;
                        rs = F.l4_off;
                        re = F.l4_off + F.l4_len;
                    }
                }
                uint64_t acc = 0;  // per lane: folded fragment partials, each at its packet parity
                uint32_t at = 0;   // packet offset of fragment j
                for (uint32_t j = f0; j < f1; ++j) {
                    const sccsum_gather_desc d = desc[j];
                    const uint32_t lo = rs > at ? rs : at;
                    const uint32_t hi = re < at + d.len ? re : at + d.len;
                    if constexpr (FILL) {  // (spos < at wraps past any length)
                        if (spos - at < d.len) saddr = frag_addr(d) + (spos - at);
                    }
                    if (lo < hi) {
                        const uintptr_t A = frag_addr(d);
                        const uint32_t head = static_cast<uint32_t>(A & 15u);
                        const uint8_t* a0 = reinterpret_cast<const uint8_t*>(A - head);
                        if (!IPV4 && hi - at >= kWideLen) {
                            // a fragment's range past the int arithmetic below (spans only: a
                            // frame's summed bytes lie in its first 65 595): 64-bit, one unit a lane
                            uint32_t f = exact_range_sum(a0, static_cast<uint64_t>(head) + (lo - at),
                                                         static_cast<uint64_t>(head) + (hi - at), lane);
                            // (exact_range_sum returns the wave's total in every lane; acc is summed
                            // over the wave again below)
                            if (lane != 0) f = 0;
                            if ((A ^ at) & 1u) f = swap16(f);
                            acc += f;
                            at += d.len;
                            continue;
                        }
                        // the summed bytes, relative to the aligned base a0
                        const int ulo = static_cast<int>(head + lo - at), uhi = static_cast<int>(head + hi - at);
                        const uint32_t c0 = static_cast<uint32_t>(ulo) >> 4;
                        const uint32_t c1 = (static_cast<uint32_t>(uhi) + 15u) >> 4;
                        uint64_t part = 0;
                        for (uint32_t g = c0; g < c1; g += U * kWave) {
                            u32x4 v[U];
    #pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const uint32_t c = g + static_cast<uint32_t>(u * kWave) + lane;
                                v[u] = c < c1 ? load_unit(a0 + 16u * c) : u32x4{0, 0, 0, 0};
                            }
                            if constexpr (FILL) {
                                // [xl, xh) relative to a0, like ulo / uhi; only a group that holds
                                // some of those bytes pays for the second mask (the byte masks are
                                // most of this kernel's ALU work: with both on every unit the
                                // HBM-resident fill ran 1.3x the verify)
                                const int el = static_cast<int>(head + xl) - static_cast<int>(at);
                                const int eh = static_cast<int>(head + xh) - static_cast<int>(at);
                                const int g16 = 16 * static_cast<int>(g);
                                const bool cut = el < uhi && eh > ulo && el < g16 + 16 * U * kWave && eh > g16;
                                if (cut) {
    #pragma unroll
                                    for (int u = 0; u < U; ++u) {
                                        const int c16 = 16 * static_cast<int>(g + u * kWave + lane);
                                        part += unit_sum(v[u], ulo - c16, min(uhi, el) - c16) +
                                                unit_sum(v[u], max(ulo, eh) - c16, uhi - c16);
                                    }
                                } else {
    #pragma unroll
                                    for (int u = 0; u < U; ++u) {
                                        const int c16 = 16 * static_cast<int>(g + u * kWave + lane);
                                        part += unit_sum(v[u], ulo - c16, uhi - c16);
                                    }
                                }
                            } else {
    #pragma unroll
                                for (int u = 0; u < U; ++u) {
                                    const int c16 = 16 * static_cast<int>(g + u * kWave + lane);
                                    part += unit_sum(v[u], ulo - c16, uhi - c16);
                                }
                            }
                        }
                        uint32_t f = fold16(part);
                        if ((A ^ at) & 1u) f = swap16(f);
                        acc += f;
                    }
                    at += d.len;
                }
                S = fold16(wave_sum(fold16(acc)));
            }

            if constexpr (FILL) {
                // r = the L4 value stored (0 when none is), then the stores
                uint32_t r = 0;
                if (flags & SCCSUM_FILL_L4_PSEUDO) {
                    if (put_l4) r = pseudo;
                } else if (put_l4 || echo) {
                    r = ~fold16(static_cast<uint64_t>(S) + pseudo) & 0xffffu;
                }
                const uint32_t val = (lane < 2u ? ipc : (lane < 4u ? r : 0u)) >> (8u * (lane & 1u));
#ifndef SCCSUM_AB_FILL_DESC_NOSTORE  // (A/B only: generate without the field stores, to see what they cost)
                if (son && saddr) *gst(reinterpret_cast<uint8_t*>(saddr)) = static_cast<uint8_t>(val);
#endif
                if (lane == 0) {
                    if (out) reinterpret_cast<uint32_t*>(out)[p] = ipc | r << 16;
                    if (status) status[p] = static_cast<uint8_t>(st | ((put_l4 || echo) ? SCCSUM_ST_L4_OK : 0u));
                }
                continue;
            }
            if (IPV4) {
                S = fold16(static_cast<uint64_t>(S) + pseudo);
            } else if (seed && !raw) {
                S = fold16(static_cast<uint64_t>(S) + swap16(fold16(seed[p])));
            }
            const uint32_t r = raw ? S : ~S & 0xffffu;
            if (lane == 0) {
                if (IPV4) {
                    reinterpret_cast<uint32_t*>(out)[p] = frame_word(ipc, r, st);
                    if (status) status[p] = static_cast<uint8_t>(frame_status(ipc, r, st));
                } else {
                    out[p] = static_cast<uint16_t>(r);
                    if (status) status[p] = (!raw && r == 0) ? SCCSUM_ST_OK : 0u;
                }
            }
        }
    }
}

// sccsum_ipv4_fill's mode rules (sccsum.h): at least one bit, only known bits,
// FILL_L4_PSEUDO excludes FILL_L4 and FILL_ICMP_ECHO, FILL_TSO needs FILL_L4_PSEUDO.
bool fill_mode_ok(uint32_t mode) {
    constexpr uint32_t kAll =
        SCCSUM_FILL_IP | SCCSUM_FILL_L4 | SCCSUM_FILL_L4_PSEUDO | SCCSUM_FILL_TSO | SCCSUM_FILL_ICMP_ECHO;
    return mode != 0 && !(mode & ~kAll) && !((mode & SCCSUM_FILL_L4) && (mode & SCCSUM_FILL_L4_PSEUDO)) &&
           !((mode & SCCSUM_FILL_TSO) && !(mode & SCCSUM_FILL_L4_PSEUDO)) &&
           !((mode & SCCSUM_FILL_ICMP_ECHO) && (mode & SCCSUM_FILL_L4_PSEUDO));
}

// The public fill mode's summing bits as the flat, row and engine kernels take them.
uint32_t fill_flags(uint32_t mode) {
    return ((mode & SCCSUM_FILL_L4) ? kFlagFillL4 : 0u) | ((mode & SCCSUM_FILL_ICMP_ECHO) ? kFlagFillIcmp : 0u) |
           ((mode & SCCSUM_FILL_IP) ? kFlagFillIp : 0u);
}

// FILL: one launch, the kernel stores the fields through the descriptors' own
// addresses (d_stage for src == NULL fragments); `mode` is the SCCSUM_FILL_*
// mode, checked before n == 0, and d_out may be NULL.  Else mode is 0.
template <bool IPV4, bool FILL = false>
int launch_desc(const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off,
                const uint32_t* d_len, const uint32_t* d_seed, const void* d_stage, uint16_t* d_out, uint8_t* d_status,
                uint64_t n, uint32_t max_len, uint32_t mode, void* stream) {
    if (FILL && !fill_mode_ok(mode)) return SCCSUM_EINVAL;
    if (n == 0) return SCCSUM_OK;
    // d_desc may be NULL (an rx burst of empty packets has no fragments): the
    // kernel then gives every packet zero fragments, so an empty one sums to
    // the empty sum and a non-empty one is SCCSUM_ST_RANGE
    if (!d_first || !d_off || !d_len || (!FILL && !d_out) || misaligned(d_desc, 8) || misaligned(d_first, 4) ||
        misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_seed, 4) || misaligned(d_out, IPV4 ? 4 : 2)) {
        return SCCSUM_EINVAL;
    }
    const LaunchTarget T(stream);
    if (T.rc != SCCSUM_OK) return T.rc;
    auto go = [&](auto kern) {
        return static_cast<int>(launch_kernel(kern, dim3(grid_for(n, T.dev)), dim3(kBlock), 0, T.s, d_desc, d_first,
                                              d_off, d_len, d_seed, static_cast<const uint8_t*>(d_stage), d_out,
                                              d_status, n, mode));
    };
    // the header-only fill modes read no payload: one unit per lane is plenty
    const bool sums = !FILL || (mode & (SCCSUM_FILL_L4 | SCCSUM_FILL_ICMP_ECHO)) != 0;
    switch (sums ? units_class(max_len) : 1) {
        case 1: return go(csum_desc_kernel<1, IPV4, FILL>);
        case 2: return go(csum_desc_kernel<2, IPV4, FILL>);
        default: return go(csum_desc_kernel<4, IPV4, FILL>);
    }
}
// (instantiated here: the fill kernels keep their place in the code object)
template int launch_desc<true, true>(const sccsum_gather_desc*, const uint32_t*, const uint64_t*, const uint32_t*,
                                     const uint32_t*, const void*, uint16_t*, uint8_t*, uint64_t, uint32_t, uint32_t,
                                     void*);

// Engine launch: the grid is what the chip holds at once (every wave's tiles
// come from the claim counters, so no block waits for another to finish).
template <bool IPV4, bool FILL = false>
hipError_t launch_engine(hipStream_t s, int dev, const EngineArgs& E, uint32_t flags, uint64_t* waves) {
    auto kern = csum_engine_kernel<16, IPV4, FILL>;
    // a multiple of 16: XCD mapping, waves divide into kGroups
    uint64_t blocks = resident_blocks(kern, dev) & ~uint64_t(15);
    if (blocks == 0) blocks = 16;
    *waves = blocks * kWavesPerBlock;
    return launch_kernel(kern, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s, E, flags);
}

}  // namespace
}  // namespace sccsum

// ---- resident engine, host side (sccsum.h "Resident engine")
struct sccsum_engine {
    int device = 0;
    bool frames = true, fill = false;
    uint32_t ring = 0;           // descriptor ring slots (a power of two >= 2)
    uint32_t max_in_flight = 0;
    uint32_t limit = 0;          // steps submitted and not done at most: min(max_in_flight, ring)
    uint64_t idle_ticks = 0, dep_ticks = 0;  // the create options, in 100 MHz ticks
    uint64_t* ring_h = nullptr;  // pinned descriptors (host view)
    uint64_t* ctl_h = nullptr;   // pinned control words (host view)
    sccsum::EngineArgs args{};   // device views + device counters
    hipStream_t stream = nullptr;
    hipEvent_t left = nullptr;   // recorded after the last run's grid: it has left once this completes
    bool launched = false, left_recorded = false;
    uint64_t waves = 0;          // the running grid's waves (tile sizing)
    void* blk = nullptr;         // the device block: claims | mirror | sdone | counts | gdone (EngineBlock)
    bool dirty = true;           // the counts / gdone words may be nonzero (a run that gave up, or none yet)
    // Producers — any number of host threads, Seastar's shards on this GPU —
    // meet under mu: a step's number, its first tile and its descriptor are
    // taken, written and published in one short critical section (no device
    // call, no wait), so steps are published in order and the grid's poller
    // never sees a hole.  Waiting for room under the in-flight limit happens
    // outside it.
    std::mutex mu;
    bool running = false;                // under mu
    std::atomic<uint64_t> next_step{0};  // written under mu; sccsum_engine_wait reads it without
    uint64_t next_first = 0;             // under mu
    uint64_t last_tiled = ~0ull;         // under mu: the latest published step with tiles (a barrier's target)
    uint64_t done_floor = 0;             // under mu: every step below it is known done
    uint32_t producer_limit = 0;         // opts.producer_in_flight (0: none)
    uint64_t run = 0;                    // under mu: this run's number, unique in the process (producer records)
};

namespace {

// The engine's device words in one block, so a run resets them with one
// memset (five took ~38 us of the timed run before the grid: r05d trace).
// claims, mirror and sdone start every run at zero; the completion counters
// (counts, gdone) return to zero by themselves as each step completes (its
// last count resets them), so they are cleared only after a run that gave up
// with steps unfinished, and at the first run.
struct EngineBlock {
    static constexpr size_t kClaims = 0;  // 64-bit claim counters, 256 B apart
    static constexpr size_t kMirror = kClaims + size_t(sccsum::kGroups) * sccsum::kHeadStride * 4u;
    static constexpr size_t kSdone = kMirror + 512u;
    static constexpr size_t kReset = kSdone + size_t(sccsum::kEngineCountSlots) * 8u * 8u;  // cleared every run
    static constexpr size_t kCounts = (kReset + 255u) & ~size_t(255);
    static constexpr size_t kGdone = kCounts + size_t(sccsum::kEngineCountSlots) * sccsum::kGroups * sccsum::kHeadStride * 4u;
    static constexpr size_t kBytes = kGdone + size_t(sccsum::kEngineCountSlots) * sccsum::kHeadStride * 4u;
    static_assert(sccsum::kMirrorWords * 8u <= kSdone - kMirror, "mirror words fit their slot");
};

// One running engine per device in this process.  A grid holds every CU of
// its device and all of their LDS while it runs, so a second grid there could
// only queue behind it (and a step submitted to it would wait on the first
// run's stop): sccsum_engine_start refuses it with SCCSUM_EBUSY.  The shards
// of one GPU share its engine instead: any number of threads may submit into
// a running engine (Seastar runs one process with a reactor thread per core,
// src/core/reactor.cc:4163; ~16 of them per GPU on an 8-GPU box).
std::mutex g_live_mu;
sccsum_engine* g_live[sccsum::kMaxDevices] = {};
std::atomic<uint64_t> g_engine_runs{0};  // numbers every run of every engine (a producer's records)

// A producer thread's own steps not yet known done, per engine run it feeds
// (opts.producer_in_flight).  Thread-local: a shard's reactor thread is the
// producer, as Seastar's shards are (src/core/reactor.cc:3437).
struct ProducerRecord {
    const sccsum_engine* e = nullptr;
    uint64_t run = 0;
    uint64_t steps[sccsum::kEngineCountSlots] = {};  // a ring of its submitted steps, oldest at head
    uint32_t head = 0, n = 0;
};
thread_local ProducerRecord t_producer[4];  // the runs this thread fed last (an engine per device at most)

ProducerRecord& producer_record(const sccsum_engine* e, uint64_t run) {
    ProducerRecord* free_one = &t_producer[0];
    for (ProducerRecord& r : t_producer) {
        if (r.e == e && r.run == run) return r;
        if (r.run < free_one->run) free_one = &r;  // the oldest run's record is reused
    }
    *free_one = ProducerRecord{};
    free_one->e = e;
    free_one->run = run;
    return *free_one;
}

void release_live(sccsum_engine* e) {
    std::lock_guard<std::mutex> g(g_live_mu);
    if (g_live[e->device] == e) g_live[e->device] = nullptr;
}

// The calling thread's current device, put back on scope exit (create must
// not leave a shard thread bound to another device: its later launches on its
// own streams would then be refused).
struct CurrentDevice {
    int dev = -1;
    CurrentDevice() {
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    }
    ~CurrentDevice() {
        if (dev >= 0) (void)hipSetDevice(dev);
    }
};

uint64_t now_ns() {
    return static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                     std::chrono::steady_clock::now().time_since_epoch())
                                     .count());
}

// Step s is done.  Its done word is a ring slot shared with s + ring,
// s + 2 ring, ...: the slot's value only rises, and s + ring is published
// only once s is done, so any value past s says so too.
bool engine_done(const sccsum_engine* e, uint64_t s) {
    return __atomic_load_n(e->ctl_h + sccsum::kEcDone + 8u * (s & (e->ring - 1u)), __ATOMIC_ACQUIRE) >= s + 1;
}

// The grid's give-up, as an error code: SCCSUM_EIDLE (no new step for the
// idle limit) or SCCSUM_EFAULT (a dependency or step lookup that could not
// finish: never expected)
int engine_error(const sccsum_engine* e) {
    const uint64_t v = __atomic_load_n(e->ctl_h + sccsum::kEcError, __ATOMIC_ACQUIRE);
    return v == 0 ? SCCSUM_OK : (v == sccsum::kErrIdle ? SCCSUM_EIDLE : SCCSUM_EFAULT);
}

// spin until step s is done, the grid gave up, or the deadline passes
int engine_wait_done(const sccsum_engine* e, uint64_t s, uint64_t timeout_ns) {
    const uint64_t t0 = now_ns();
    for (uint32_t k = 0;; ++k) {
        if (engine_done(e, s)) return SCCSUM_OK;
        if (const int rc = engine_error(e)) return rc;
        if ((k & 255u) == 255u && now_ns() - t0 > timeout_ns) return SCCSUM_EBUSY;
    }
}

// Every published step of the run is done (under mu; steps below done_floor are)
bool engine_all_done(sccsum_engine* e) {
    const uint64_t n = e->next_step.load(std::memory_order_relaxed);
    while (e->done_floor < n && engine_done(e, e->done_floor)) ++e->done_floor;
    return e->done_floor >= n;
}

// The batches of one step, checked as the launches check them.
int engine_check(const sccsum_engine* e, const sccsum_batch* batches, uint32_t nbatch, bool fill) {
    if (nbatch == 0 || nbatch > SCCSUM_ENGINE_MAX_BATCHES || !batches) return SCCSUM_EINVAL;
    for (uint32_t i = 0; i < nbatch; ++i) {
        const sccsum_batch& x = batches[i];
        if (e->frames && x.d_seed) return SCCSUM_EINVAL;  // frames derive their pseudo-header in-kernel
        if (!x.n) continue;
        const bool ok = e->frames
                            ? sccsum::batch_ok<true>(x.d_bytes, x.d_off, x.d_len, nullptr, x.d_out, x.d_status, 0)
                            : sccsum::batch_ok<false>(x.d_bytes, x.d_off, x.d_len, x.d_seed, x.d_out, x.d_status, 0);
        if (!ok) return SCCSUM_EINVAL;
        if (fill && !x.d_out) return SCCSUM_EINVAL;  // a fill's values pass from its generate to its store step
    }
    return SCCSUM_OK;
}

// Room (under mu) to publish k more steps now: every step up to `limit`
// before the last of them is done — not only that one: steps finish out of
// order (a small step behind a big one's last tile).  That also frees what
// the new steps take over: their descriptor ring slots and done words (slot
// s & (ring - 1), limit <= ring) and their completion counters (slot s %
// kEngineCountSlots, limit <= kEngineCountSlots).  Else *need = the step to
// wait for.  A caller may also free an older step's buffers once a later
// submit returns.
bool engine_room(sccsum_engine* e, uint32_t k, uint64_t* need) {
    const uint64_t last = e->next_step.load(std::memory_order_relaxed) + k - 1;
    if (last < e->limit) return true;
    const uint64_t target = last - e->limit;
    while (e->done_floor <= target && engine_done(e, e->done_floor)) ++e->done_floor;
    if (e->done_floor > target) return true;
    *need = e->done_floor;
    return false;
}

// Packets per tile of a summing step, the function a launch picks them with
// (packets_per_tile), over the running grid's waves.  The mean packet is the
// batches' bytes over their packets, capped by max_len when the caller gives
// it (packet_bytes): a batch that is a slice of a larger buffer (bytes_len
// covers the whole buffer) would otherwise look sparse and get tiles of a
// packet or two.  (The knobs are the submitting thread's.)
uint64_t engine_tile(const sccsum_engine* e, const sccsum_batch* batches, uint32_t nbatch, uint32_t max_len) {
    uint64_t n_total = 0, bytes_total = 0;
    for (uint32_t i = 0; i < nbatch; ++i) {
        n_total += batches[i].n;
        bytes_total += batches[i].n ? batches[i].bytes_len : 0;
    }
    return sccsum::packets_per_tile(n_total, sccsum::packet_bytes(n_total, bytes_total, max_len), e->waves,
                                    sccsum::t_knobs);
}

// Write one step's descriptor over checked batches (nbatch 0: an empty step,
// done at once) into its ring slot and publish it (under mu; engine_room made
// the room).  kind = the descriptor's kind word, dep = 0 or 1 + the step its
// tiles wait for, B = packets per tile of a summing step (engine_tile); a
// store step's tiles always hold kStoreTilePackets frames.
uint64_t engine_put(sccsum_engine* e, const sccsum_batch* batches, uint32_t nbatch, uint64_t kind, uint64_t dep,
                    uint64_t B) {
    if ((kind & 0xffu) == sccsum::kStepFillStore) B = sccsum::kStoreTilePackets;  // four frames per lane
    const uint64_t s = e->next_step.load(std::memory_order_relaxed);
    uint64_t* const d = e->ring_h + (s & (e->ring - 1u)) * sccsum::kEngineSlotWords;
    uint64_t tile0[SCCSUM_ENGINE_MAX_BATCHES + 1] = {};
    uint32_t nq = 0;
    for (uint32_t i = 0; i < nbatch; ++i) {
        const sccsum_batch& x = batches[i];
        if (!x.n) continue;
        const uint32_t q = nq++;
        uint64_t* w = d + sccsum::kEdQueue + 8u * q;
        w[0] = reinterpret_cast<uint64_t>(x.d_bytes);
        w[1] = x.bytes_len;
        w[2] = reinterpret_cast<uint64_t>(x.d_off);
        w[3] = reinterpret_cast<uint64_t>(x.d_len);
        w[4] = e->frames ? 0u : reinterpret_cast<uint64_t>(x.d_seed);
        w[5] = reinterpret_cast<uint64_t>(x.d_out);
        w[6] = reinterpret_cast<uint64_t>(x.d_status);
        w[7] = x.n;
        tile0[q + 1] = tile0[q] + (x.n + B - 1) / B;
    }
    const uint64_t ntiles = tile0[nq];
    d[sccsum::kEdFirst] = e->next_first;
    d[sccsum::kEdTiles] = ntiles | (B << 32);
    d[sccsum::kEdStep] = sccsum::engine_seal(s, e->next_first + ntiles);
    d[sccsum::kEdIndex] = s;
    d[sccsum::kEdNq] = nq ? nq : 1;
    for (uint32_t q = 0; q <= SCCSUM_ENGINE_MAX_BATCHES; ++q) d[sccsum::kEdTile0 + q] = tile0[q];
    d[sccsum::kEdKind] = kind;
    d[sccsum::kEdDep] = dep;
    // Re-synchronise the grid every k steps: the step's tiles wait for the one
    // before it, so dequeue groups that drifted apart line up again.  A grid
    // of fixed groups drifts over a long run: cfg 2's
    // 200-step run took 457-458 us per step unsynchronised, 448-449 with a
    // barrier every 10 steps, 456 with one every step, and launches 461
    // (profiles/r05_engine_sync.log).  By default only big steps (>= 2 tiles
    // per wave) synchronise; a stream of small steps keeps its pipeline full.
    int sync = sccsum::t_knobs.engine_sync_every;
    if (sync < 0) sync = ntiles >= 2 * e->waves ? static_cast<int>(sccsum::kEngineSyncEvery) : 0;
    // The barrier waits for the latest step with tiles: a step without tiles
    // is marked done in host memory only (by the poller, once copied), and its
    // device done word never rises, so waiting on it would hold the grid until
    // the dependency limit (fuzz case 35 at 16x: a barrier step behind an
    // empty step).
    if (dep == 0 && sync > 0 && s > 0 && s % static_cast<uint64_t>(sync) == 0 && e->last_tiled != ~0ull) {
        d[sccsum::kEdDep] = e->last_tiled + 1;
    }
    if (ntiles) e->last_tiled = s;
    // (a step without tiles is done when the grid's poller has copied it: its
    // host slot is free again only then)
    e->next_first += ntiles;
    e->next_step.store(s + 1, std::memory_order_release);
    // publish: the descriptor is complete before the grid's poller can see the step
    __atomic_store_n(e->ctl_h + sccsum::kEcPublished, s + 1, __ATOMIC_SEQ_CST);
    return s;
}

// Publish k (1 or 2) steps together through put() once there is room,
// waiting for room outside the lock (other producers publish meanwhile).
// With a per-producer limit the calling thread first waits, outside the
// lock, until fewer than that many of its own steps are pending.
template <class Put>
int engine_publish(sccsum_engine* e, uint32_t k, uint64_t timeout_ns, const Put& put) {
    const uint64_t t0 = now_ns();
    ProducerRecord* pr = nullptr;
    if (e->producer_limit) {
        uint64_t run;
        {
            std::lock_guard<std::mutex> g(e->mu);
            if (!e->running) return SCCSUM_EINVAL;
            run = e->run;
        }
        pr = &producer_record(e, run);
        while (pr->n >= e->producer_limit) {
            const uint64_t oldest = pr->steps[pr->head];
            const uint64_t spent = now_ns() - t0;
            const int rc = engine_wait_done(e, oldest, spent < timeout_ns ? timeout_ns - spent : 0);
            if (rc != SCCSUM_OK) return rc;
            pr->head = (pr->head + 1) % sccsum::kEngineCountSlots;
            --pr->n;
        }
    }
    for (;;) {
        uint64_t need = 0;
        {
            std::lock_guard<std::mutex> g(e->mu);
            if (!e->running) return SCCSUM_EINVAL;  // not started, or stopped: nothing would run the step
            if (const int rc = engine_error(e)) return rc;
            if (engine_room(e, k, &need)) {
                put();
                if (pr) {  // the put's last step (a fill's store step) stands for it
                    pr->steps[(pr->head + pr->n) % sccsum::kEngineCountSlots] =
                        e->next_step.load(std::memory_order_relaxed) - 1;
                    ++pr->n;
                }
                return SCCSUM_OK;
            }
        }
        const uint64_t spent = now_ns() - t0;
        const int rc = engine_wait_done(e, need, spent < timeout_ns ? timeout_ns - spent : 0);
        if (rc != SCCSUM_OK) return rc;
    }
}

int engine_ms(uint32_t ms, uint32_t dflt, uint64_t* ticks) {
    const uint64_t v = ms ? ms : dflt;
    if (v > 3600000u) return SCCSUM_EINVAL;
    *ticks = v * 100000ull;  // the constant 100 MHz clock
    return SCCSUM_OK;
}

}  // namespace

extern "C" {

int sccsum_engine_create_opts(int device, int mode, const sccsum_engine_opts* opts, sccsum_engine** out) {
    const int base = mode & ~SCCSUM_ENGINE_FILL;
    const bool fill = (mode & SCCSUM_ENGINE_FILL) != 0;
    if (!out || !opts || (base != SCCSUM_PIPE_IPV4 && base != SCCSUM_PIPE_SPANS) || (fill && base != SCCSUM_PIPE_IPV4)) {
        return SCCSUM_EINVAL;
    }
    const uint32_t ring_req = opts->ring_slots ? opts->ring_slots : sccsum::kEngineDefaultRing;
    const uint32_t mif = opts->max_in_flight ? opts->max_in_flight : 8u;
    uint64_t idle_ticks = 0, dep_ticks = 0;
    if (ring_req > sccsum::kEngineMaxRing || mif > sccsum::kEngineCountSlots || (fill && mif < 2) ||
        opts->producer_in_flight > mif ||
        engine_ms(opts->idle_ms, 1000u, &idle_ticks) != SCCSUM_OK || engine_ms(opts->dep_ms, 2000u, &dep_ticks) != SCCSUM_OK) {
        return SCCSUM_EINVAL;
    }
    uint32_t ring = 2;
    while (ring < ring_req) ring <<= 1;
    *out = nullptr;
    int n = 0;
    hipError_t e0 = hipGetDeviceCount(&n);
    if (e0 != hipSuccess) return static_cast<int>(e0);
    if (device < 0 || device >= n || device >= sccsum::kMaxDevices) return SCCSUM_ENODEV;
    const CurrentDevice keep;  // the allocations go to `device`; the caller's binding is put back
    if ((e0 = hipSetDevice(device)) != hipSuccess) return static_cast<int>(e0);
    auto* e = new (std::nothrow) sccsum_engine;
    if (!e) return static_cast<int>(hipErrorOutOfMemory);
    e->device = device;
    e->frames = base == SCCSUM_PIPE_IPV4;
    e->fill = fill;
    e->ring = ring;
    e->max_in_flight = mif;
    e->limit = mif < ring ? mif : ring;
    e->idle_ticks = idle_ticks;
    e->dep_ticks = dep_ticks;
    e->producer_limit = opts->producer_in_flight;
    const uint64_t ring_bytes = uint64_t(ring) * sccsum::kEngineSlotWords * 8u;
    const uint64_t ctl_bytes = (sccsum::kEcDone + 8u * uint64_t(ring)) * 8u;
    const unsigned fl = hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable;
    void *rh = nullptr, *ch = nullptr, *rd = nullptr, *cd = nullptr, *bk = nullptr, *dr = nullptr;
    hipError_t r = hipHostMalloc(&rh, ring_bytes, fl);
    if (r == hipSuccess) r = hipHostMalloc(&ch, ctl_bytes, fl);
    if (r == hipSuccess) r = hipHostGetDevicePointer(&rd, rh, 0);
    if (r == hipSuccess) r = hipHostGetDevicePointer(&cd, ch, 0);
    if (r == hipSuccess) r = hipMalloc(&bk, EngineBlock::kBytes);
    if (r == hipSuccess) r = hipMalloc(&dr, ring_bytes);
    if (r == hipSuccess) r = hipEventCreateWithFlags(&e->left, hipEventDisableTiming);
    if (r != hipSuccess) {
        for (void* p : {rh, ch}) if (p) (void)hipHostFree(p);
        for (void* p : {bk, dr}) if (p) (void)hipFree(p);
        delete e;
        return static_cast<int>(r);
    }
    std::memset(rh, 0, ring_bytes);
    std::memset(ch, 0, ctl_bytes);
    e->ring_h = static_cast<uint64_t*>(rh);
    e->ctl_h = static_cast<uint64_t*>(ch);
    e->args.hring = static_cast<const uint64_t*>(rd);
    e->args.dring = static_cast<uint64_t*>(dr);
    e->args.ring_mask = ring - 1u;
    e->args.ctl = static_cast<uint64_t*>(cd);
    e->blk = bk;
    uint8_t* const b = static_cast<uint8_t*>(bk);
    e->args.claims = reinterpret_cast<uint64_t*>(b + EngineBlock::kClaims);
    e->args.mirror = reinterpret_cast<uint64_t*>(b + EngineBlock::kMirror);
    e->args.sdone = reinterpret_cast<uint64_t*>(b + EngineBlock::kSdone);
    e->args.counts = reinterpret_cast<uint32_t*>(b + EngineBlock::kCounts);
    e->args.gdone = reinterpret_cast<uint32_t*>(b + EngineBlock::kGdone);
    e->args.idle_ticks = idle_ticks;
    e->args.dep_ticks = dep_ticks;
    *out = e;
    return SCCSUM_OK;
}

int sccsum_engine_create(int device, int mode, uint32_t max_steps, uint32_t max_in_flight, sccsum_engine** out) {
    if (max_steps == 0 || max_in_flight == 0) return SCCSUM_EINVAL;
    const sccsum_engine_opts o = {max_steps, max_in_flight, 0u, 0u};
    return sccsum_engine_create_opts(device, mode, &o, out);
}

int sccsum_engine_start(sccsum_engine* e, void* stream) {
    if (!e) return SCCSUM_EINVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (e->running) return SCCSUM_EINVAL;
    const sccsum::LaunchTarget T(stream);
    if (T.rc != SCCSUM_OK) return T.rc;
    const hipStream_t s = T.s;
    const int dev = T.dev;
    if (dev != e->device) return SCCSUM_EINVAL;
    {
        std::lock_guard<std::mutex> gl(g_live_mu);
        if (g_live[dev] != nullptr) return SCCSUM_EBUSY;  // another engine's run holds the device
        g_live[dev] = e;
    }
    // the last run's grid has left (stop only asks it to): its control words are ours again
    if (e->launched) {
        const hipError_t w = e->left_recorded ? hipEventSynchronize(e->left) : hipStreamSynchronize(e->stream);
        if (w != hipSuccess) {
            release_live(e);
            return static_cast<int>(w);
        }
    }
    // a new run: no step published, none done, counters zero (stream-ordered before the grid).
    // A run that gave up (EIDLE, a fault) may have left completion counters behind.
    if (__atomic_load_n(e->ctl_h + sccsum::kEcError, __ATOMIC_ACQUIRE)) e->dirty = true;
    const uint64_t used = e->next_step.load(std::memory_order_relaxed);  // the done words the last run wrote
    std::memset(e->ctl_h, 0, (sccsum::kEcDone + 8u * (used < e->ring ? used : e->ring)) * 8u);
    std::atomic_thread_fence(std::memory_order_seq_cst);
    hipError_t r = hipMemsetAsync(e->blk, 0, e->dirty ? EngineBlock::kBytes : EngineBlock::kReset, s);
    if (r != hipSuccess) {
        release_live(e);
        return static_cast<int>(r);
    }
    const sccsum::Knobs& K = sccsum::t_knobs;
    const uint32_t flags = sccsum::knob_flags(K) | (K.engine_wt ? sccsum::kFlagEngineWT : 0u);
    // the engine's idle limit, unless this thread's diagnostic knob overrides it
    e->args.idle_ticks = K.engine_idle_ms > 0 ? static_cast<uint64_t>(K.engine_idle_ms) * 100000ull : e->idle_ticks;
    r = e->fill ? sccsum::launch_engine<true, true>(s, dev, e->args, flags, &e->waves)
                : (e->frames ? sccsum::launch_engine<true>(s, dev, e->args, flags, &e->waves)
                             : sccsum::launch_engine<false>(s, dev, e->args, flags, &e->waves));
    if (r != hipSuccess) {
        release_live(e);
        return static_cast<int>(r);
    }
    e->left_recorded = hipEventRecord(e->left, s) == hipSuccess;  // else the next start syncs the stream
    e->launched = true;
    e->stream = s;
    e->running = true;
    e->next_step.store(0, std::memory_order_release);
    e->next_first = 0;
    e->last_tiled = ~0ull;
    e->done_floor = 0;
    e->run = g_engine_runs.fetch_add(1, std::memory_order_relaxed) + 1;
    e->dirty = false;  // (until this run is found to have given up)
    return SCCSUM_OK;
}

int sccsum_engine_submit(sccsum_engine* e, const sccsum_batch* batches, uint32_t nbatch, uint32_t max_len,
                         uint64_t timeout_ns, uint64_t* step) {
    if (!e || !step) return SCCSUM_EINVAL;
    if (const int rc = engine_check(e, batches, nbatch, false); rc != SCCSUM_OK) return rc;
    return engine_publish(e, 1, timeout_ns, [&] {
        *step = engine_put(e, batches, nbatch, sccsum::kStepSum, 0, engine_tile(e, batches, nbatch, max_len));
    });
}

// In-place fill as two steps published together: the generate step, then the
// store step whose tiles wait for it.  Both or neither: the room for two is
// made first (max_in_flight >= 2 for a fill engine, so that wait never waits
// on the generate step itself).  The store step right behind its generate
// step runs as a phase of its own: its waves wait out the generate step's
// drain (~10-18 us) and then store with few reads beside them.  Deferred
// behind the next fill's generate step instead (no drain wait), the store
// tiles of the groups that finished first ran inside the other groups' read
// stream, and a fill took 354-356 us against 328 (profiles/r05_engine_fill.log).
int sccsum_engine_submit_fill(sccsum_engine* e, const sccsum_batch* batches, uint32_t nbatch, uint32_t max_len,
                              uint32_t mode, uint64_t timeout_ns, uint64_t* step) {
    constexpr uint32_t kEngineModes = SCCSUM_FILL_IP | SCCSUM_FILL_L4 | SCCSUM_FILL_ICMP_ECHO;
    if (!e || !step || !e->fill || (mode & ~kEngineModes) || !(mode & (SCCSUM_FILL_L4 | SCCSUM_FILL_ICMP_ECHO))) {
        return SCCSUM_EINVAL;
    }
    if (const int rc = engine_check(e, batches, nbatch, true); rc != SCCSUM_OK) return rc;
    uint64_t n_total = 0;
    for (uint32_t i = 0; i < nbatch; ++i) n_total += batches[i].n;
    // a small fill is one step whose tiles store their own fields (no store
    // step, no wait on the generate step: a store step's waves hold the next
    // fill's tiles while they wait, which chained small fills one after another)
    const bool single = n_total <= sccsum::t_knobs.fill_single_max;
    const uint64_t kflags = sccsum::fill_flags(mode) | (single ? sccsum::kFlagFillNow : 0u);
    const uint64_t gen_kind = sccsum::kStepFillGen | (kflags << 8) | (uint64_t(mode) << 16);
    if (single) {
        return engine_publish(e, 1, timeout_ns, [&] {
            *step = engine_put(e, batches, nbatch, gen_kind, 0, engine_tile(e, batches, nbatch, max_len));
        });
    }
    // (cutting a 1 Mi-frame fill into two one-pass steps of 512 Ki did not help:
    // 343.6 us a fill against 330 in two passes; profiles/r05_fill_one_pass.log)
    // the store half: no status (the generate half reported it)
    sccsum_batch st[SCCSUM_ENGINE_MAX_BATCHES];
    for (uint32_t i = 0; i < nbatch; ++i) {
        st[i] = batches[i];
        st[i].d_status = nullptr;
    }
    return engine_publish(e, 2, timeout_ns, [&] {
        const uint64_t gen = engine_put(e, batches, nbatch, gen_kind, 0, engine_tile(e, batches, nbatch, max_len));
        *step = engine_put(e, st, nbatch, sccsum::kStepFillStore | (uint64_t(mode) << 16), gen + 1, 0);
    });
}

int sccsum_engine_wait(sccsum_engine* e, uint64_t step, uint64_t timeout_ns) {
    if (!e || step >= e->next_step.load(std::memory_order_acquire)) return SCCSUM_EINVAL;
    return engine_wait_done(e, step, timeout_ns);
}

int sccsum_engine_stop(sccsum_engine* e) {
    if (!e) return SCCSUM_EINVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->running) return SCCSUM_EINVAL;
    __atomic_store_n(e->ctl_h + sccsum::kEcStop, 1ull, __ATOMIC_SEQ_CST);  // after every published step (mu)
    e->running = false;
    release_live(e);  // the grid leaves once the published steps are done
    // the grid gave up before the call with published steps not (yet) done
    const int err = engine_error(e);
    return err && !engine_all_done(e) ? err : SCCSUM_OK;
}

int sccsum_engine_destroy(sccsum_engine* e) {
    if (!e) return SCCSUM_OK;
    bool running;
    {
        std::lock_guard<std::mutex> g(e->mu);
        running = e->running;
    }
    if (running) (void)sccsum_engine_stop(e);
    int rc = e->stream ? static_cast<int>(hipStreamSynchronize(e->stream)) : SCCSUM_OK;
    // The grid has left: a published step that is not done was lost (ADVICE
    // r05: an idle give-up after every step was done loses nothing)
    if (rc == SCCSUM_OK && e->launched) {
        std::lock_guard<std::mutex> g(e->mu);
        if (!engine_all_done(e)) rc = engine_error(e) ? engine_error(e) : SCCSUM_EFAULT;
    }
    (void)hipHostFree(e->ring_h);
    (void)hipHostFree(e->ctl_h);
    (void)hipFree(e->blk);
    (void)hipFree(e->args.dring);
    if (e->left) (void)hipEventDestroy(e->left);
    delete e;
    return rc;
}

int sccsum_abi_version(void) { return SCCSUM_ABI_VERSION; }

const char* sccsum_strerror(int err) {
    if (err == SCCSUM_OK) return "success";
    if (err == SCCSUM_EINVAL) return "invalid argument";
    if (err == SCCSUM_ENODEV) return "no such HIP device";
    if (err == SCCSUM_EBUSY) return "busy: every batch slot or engine step is in flight, or the device's engine is running";
    if (err == SCCSUM_EIDLE) return "the engine's grid gave up waiting for steps";
    if (err == SCCSUM_EFAULT) return "the engine's grid stopped on an internal fault";
    if (err > 0) return hipGetErrorString(static_cast<hipError_t>(err));
    return "unknown sccsum error";
}

int sccsum_device_count(int* count) {
    if (!count) return SCCSUM_EINVAL;
    return static_cast<int>(hipGetDeviceCount(count));
}

int sccsum_device_numa_node(int device, int* node) {
    if (!node) return SCCSUM_EINVAL;
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return static_cast<int>(e);
    if (device < 0 || device >= n) return SCCSUM_ENODEV;
    char bdf[64] = {};
    const hipError_t e2 = hipDeviceGetPCIBusId(bdf, static_cast<int>(sizeof(bdf)), device);
    if (e2 != hipSuccess) return static_cast<int>(e2);
    for (char* c = bdf; *c; ++c) *c = static_cast<char>(std::tolower(static_cast<unsigned char>(*c)));
    char path[160];
    std::snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
    *node = -1;
    if (FILE* f = std::fopen(path, "r")) {
        int v = -1;
        if (std::fscanf(f, "%d", &v) == 1) *node = v;
        std::fclose(f);
    }
    return SCCSUM_OK;
}

int sccsum_init(int device) {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return static_cast<int>(e);
    if (device < 0 || device >= n) return SCCSUM_ENODEV;
    const hipError_t e2 = hipSetDevice(device);
    if (e2 != hipSuccess) return static_cast<int>(e2);
    (void)sccsum::cu_count(device);
    return sccsum::ensure_heads(device);
}

// ip.hh:70-75 via checksummer::sum_many(uint32 src, uint32 dst, uint8 0,
// uint8 proto, uint16 len) from a fresh (even) checksummer: the uint8 pair
// forms the big-endian word (0, proto); everything is added as host integers.
uint32_t sccsum_pseudo_seed(uint32_t src_host, uint32_t dst_host, uint8_t proto, uint16_t len) {
    uint64_t s = static_cast<uint64_t>(src_host) + dst_host + proto + len;
    while (s >> 16) s = (s & 0xffffu) + (s >> 16);
    return static_cast<uint32_t>(s);
}

int sccsum_spans(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                 const uint32_t* d_seed, uint16_t* d_out, uint8_t* d_status, uint64_t n, uint32_t max_len,
                 void* stream) {
    return sccsum::launch<false>(d_bytes, bytes_len, d_off, d_len, d_seed, d_out, d_status, n, max_len, stream);
}

int sccsum_ipv4_frames(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                       uint16_t* d_out2, uint8_t* d_status, uint64_t n, uint32_t max_len, void* stream) {
    return sccsum::launch<true>(d_bytes, bytes_len, d_off, d_len, nullptr, d_out2, d_status, n, max_len, stream);
}

int sccsum_spans_multi(const sccsum_batch* batches, uint32_t nbatch, uint32_t max_len, void* stream) {
    return sccsum::launch_multi<false>(batches, nbatch, max_len, stream);
}

int sccsum_ipv4_frames_multi(const sccsum_batch* batches, uint32_t nbatch, uint32_t max_len, void* stream) {
    return sccsum::launch_multi<true>(batches, nbatch, max_len, stream);
}

static int rss_args_ok(const uint8_t* key, uint32_t key_len, int mode, const uint32_t* d_hash) {
    return key && key_len >= 4 && (mode == SCCSUM_RSS_DISPATCH || mode == SCCSUM_RSS_REASSEMBLED) && d_hash &&
           !sccsum::misaligned(d_hash, 4);
}

int sccsum_ipv4_rss(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                    const uint8_t* key, uint32_t key_len, int mode, uint32_t* d_hash, uint8_t* d_status, uint64_t n,
                    void* stream) {
    if (n == 0) return SCCSUM_OK;
    if (!rss_args_ok(key, key_len, mode, d_hash) || !d_bytes || !d_off || !d_len || sccsum::misaligned(d_bytes, 16) ||
        sccsum::misaligned(d_off, 8) || sccsum::misaligned(d_len, 4)) {
        return SCCSUM_EINVAL;
    }
    const sccsum::LaunchTarget T(stream);
    if (T.rc != SCCSUM_OK) return T.rc;
    const sccsum::RssParams P = sccsum::make_rss(key, key_len, static_cast<uint32_t>(mode), d_hash);
    return static_cast<int>(sccsum::launch_kernel(sccsum::rss_kernel, dim3(sccsum::blocks_for(n)),
                                                  dim3(sccsum::kBlock), 0, T.s, static_cast<const uint8_t*>(d_bytes),
                                                  bytes_len, d_off, d_len, d_status, n, P));
}

int sccsum_ipv4_frames_rss(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                           uint16_t* d_out2, uint8_t* d_status, uint64_t n, uint32_t max_len, const uint8_t* key,
                           uint32_t key_len, int rss_mode, uint32_t* d_hash, void* stream) {
    if (n == 0) return SCCSUM_OK;
    if (!rss_args_ok(key, key_len, rss_mode, d_hash)) return SCCSUM_EINVAL;
    const sccsum::RssParams P = sccsum::make_rss(key, key_len, static_cast<uint32_t>(rss_mode), d_hash);
    return sccsum::launch<true>(d_bytes, bytes_len, d_off, d_len, nullptr, d_out2, d_status, n, max_len, stream, 0u,
                                P);
}

int sccsum_gather(const sccsum_gather_desc* d_desc, uint64_t n, void* d_dst, void* stream) {
    if (n == 0) return SCCSUM_OK;
    if (!d_desc || !d_dst || sccsum::misaligned(d_desc, 8)) return SCCSUM_EINVAL;
    const sccsum::LaunchTarget T(stream);
    if (T.rc != SCCSUM_OK) return T.rc;
    const uint64_t blocks = std::min<uint64_t>((n + 3) / 4, 65536);
    return static_cast<int>(sccsum::launch_kernel(sccsum::gather_kernel, dim3(static_cast<unsigned>(blocks)),
                                                  dim3(sccsum::kBlock), 0, T.s, d_desc, n,
                                                  static_cast<uint8_t*>(d_dst)));
}

int sccsum_spans_desc(const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off,
                      const uint32_t* d_len, const uint32_t* d_seed, const void* d_stage, uint16_t* d_out,
                      uint8_t* d_status, uint64_t n, uint32_t max_len, void* stream) {
    return sccsum::launch_desc<false>(d_desc, d_first, d_off, d_len, d_seed, d_stage, d_out, d_status, n, max_len, 0,
                                      stream);
}

int sccsum_ipv4_frames_desc(const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off,
                            const uint32_t* d_len, const void* d_stage, uint16_t* d_out2, uint8_t* d_status,
                            uint64_t n, uint32_t max_len, void* stream) {
    return sccsum::launch_desc<true>(d_desc, d_first, d_off, d_len, nullptr, d_stage, d_out2, d_status, n, max_len, 0,
                                     stream);
}

int sccsum_ipv4_fill_desc(const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off,
                          const uint32_t* d_len, void* d_stage, uint16_t* d_out2, uint8_t* d_status, uint64_t n,
                          uint32_t max_len, uint32_t mode, void* stream) {
    return sccsum::launch_desc<true, true>(d_desc, d_first, d_off, d_len, nullptr, d_stage, d_out2, d_status, n,
                                           max_len, mode, stream);
}

uint64_t sccsum_fragments_workspace(uint64_t nfrag) { return ((2 * nfrag + 15) & ~uint64_t(15)) + nfrag + 16; }

int sccsum_fragments(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_frag_off, const uint32_t* d_frag_len,
                     uint64_t nfrag, const uint32_t* d_pkt_first, const uint32_t* d_seed, uint16_t* d_out,
                     uint8_t* d_status, uint64_t n, uint32_t max_frag_len, void* d_workspace, void* stream) {
    if (n == 0) return SCCSUM_OK;
    if (!d_pkt_first || !d_out || (nfrag && (!d_workspace || !d_frag_off || !d_frag_len)) ||
        sccsum::misaligned(d_workspace, 16) || sccsum::misaligned(d_pkt_first, 4) || sccsum::misaligned(d_seed, 4) ||
        sccsum::misaligned(d_out, 2)) {
        return SCCSUM_EINVAL;
    }
    const sccsum::LaunchTarget T(stream);
    if (T.rc != SCCSUM_OK) return T.rc;
    auto* raw = static_cast<uint16_t*>(d_workspace);
    auto* raw_st = static_cast<uint8_t*>(d_workspace) + ((2 * nfrag + 15) & ~uint64_t(15));
    if (nfrag) {
        const int rc = sccsum::launch<false>(d_bytes, bytes_len, d_frag_off, d_frag_len, nullptr, raw, raw_st, nfrag,
                                             max_frag_len, stream, sccsum::kFlagRaw);
        if (rc != SCCSUM_OK) return rc;
    }
    return static_cast<int>(sccsum::launch_kernel(sccsum::frag_combine_kernel, dim3(sccsum::blocks_for(n)),
                                                  dim3(sccsum::kBlock), 0, T.s, d_frag_len, nfrag, d_pkt_first, raw,
                                                  raw_st, d_seed, d_out, d_status, n));
}

int sccsum_ipv4_fill(void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                     uint16_t* d_out2, uint8_t* d_status, uint64_t n, uint32_t max_len, uint32_t mode,
                     void* stream) {
    if (!sccsum::fill_mode_ok(mode)) return SCCSUM_EINVAL;
    if (n == 0) return SCCSUM_OK;
    const bool two_pass = (mode & (SCCSUM_FILL_L4 | SCCSUM_FILL_ICMP_ECHO)) != 0;
    if (two_pass ? !sccsum::batch_ok<true>(d_bytes, d_off, d_len, nullptr, d_out2, d_status, sccsum::kFlagFillL4)
                 : (!d_bytes || !d_off || !d_len || sccsum::misaligned(d_off, 8) || sccsum::misaligned(d_len, 4) ||
                    sccsum::misaligned(d_out2, 4))) {
        return SCCSUM_EINVAL;  // (before any allocation)
    }
    const sccsum::LaunchTarget T(stream);
    if (T.rc != SCCSUM_OK) return T.rc;
    if (two_pass && n <= sccsum::t_knobs.fill_single_max) {
        // a small fill in one pass: the generate tiles store the fields
        // themselves (kFlagFillNow; d_out2 stays optional, nothing to hand over)
        const uint32_t flags = sccsum::fill_flags(mode) | sccsum::kFlagFillNow;
        // a small one on the row kernel, as small verifies run (launch()), when
        // max_len says its frames fit the exact fast path (128 KiB).  max_len is
        // only a hint: a longer frame there is summed by the row kernel's exact
        // redo, its header read from the frame, just more slowly
        if (sccsum::t_knobs.variant == 0 && n <= sccsum::kSmallRowsMax && max_len != 0 && max_len <= sccsum::kExactMax) {
            return static_cast<int>(sccsum::launch_rows<true, false, true>(
                max_len, T.s, T.dev, static_cast<const uint8_t*>(d_bytes), bytes_len, d_off, d_len, nullptr, d_out2,
                d_status, n, flags));
        }
        return sccsum::launch<true>(d_bytes, bytes_len, d_off, d_len, nullptr, d_out2, d_status, n, max_len, stream,
                                    flags);
    }
    if (two_pass) {
        // pass 1 generates into d_out2, pass 2 stores the fields.  Without a
        // caller's d_out2 the values go through a stream-ordered allocation
        // (hipMallocAsync / hipFreeAsync on `stream`: no host sync, safe
        // under graph capture, freed once pass 2 is done with it)
        void* scratch = nullptr;
        if (!d_out2) {
            const hipError_t e = hipMallocAsync(&scratch, 4 * n, T.s);
            if (e != hipSuccess) return static_cast<int>(e);
        }
        uint16_t* const vals = d_out2 ? d_out2 : static_cast<uint16_t*>(scratch);
        int rc = sccsum::launch<true>(d_bytes, bytes_len, d_off, d_len, nullptr, vals, d_status, n, max_len,
                                      stream, sccsum::fill_flags(mode));
#ifdef SCCSUM_AB_FILL_GEN_ONLY
        if (false) {  // A/B only: the generate pass alone (the frames are not written)
#else
        if (rc == SCCSUM_OK) {
#endif
            rc = static_cast<int>(sccsum::launch_kernel(sccsum::fill_store_kernel, dim3(sccsum::blocks_for(n)),
                                                        dim3(sccsum::kBlock), 0, T.s, static_cast<uint8_t*>(d_bytes),
                                                        bytes_len, d_off, d_len,
                                                        reinterpret_cast<const uint32_t*>(vals), n, mode));
        }
        if (scratch) {
            const hipError_t e = hipFreeAsync(scratch, T.s);
            if (rc == SCCSUM_OK && e != hipSuccess) rc = static_cast<int>(e);
        }
        return rc;
    }
    return static_cast<int>(sccsum::launch_kernel(sccsum::fill_header_kernel, dim3(sccsum::blocks_for(n)),
                                                  dim3(sccsum::kBlock), 0, T.s, static_cast<uint8_t*>(d_bytes),
                                                  bytes_len, d_off, d_len, reinterpret_cast<uint32_t*>(d_out2),
                                                  d_status, n, mode));
}

int sccsum_set_kernel_variant(int variant) {
    if (!(variant == 0 || variant == 1 || variant == 2 || (variant >= 14 && variant <= 16))) return SCCSUM_EINVAL;
    sccsum::t_knobs.variant = variant;
    return SCCSUM_OK;
}

int sccsum_set_blocks_per_cu(int blocks) {
    if (blocks < 1 || blocks > 32) return SCCSUM_EINVAL;
    sccsum::t_knobs.blocks_per_cu = blocks;
    return SCCSUM_OK;
}

int sccsum_set_group_units(int units) {
    if (units != 0 && units != 1 && units != 2 && units != 4 && units != 8) return SCCSUM_EINVAL;
    sccsum::t_knobs.group_units = units;
    return SCCSUM_OK;
}

int sccsum_set_fill_single_max(int frames) {
    if (frames < 0) return SCCSUM_EINVAL;
    sccsum::t_knobs.fill_single_max = static_cast<uint32_t>(frames);
    return SCCSUM_OK;
}

int sccsum_set_tile_packets(int packets) {
    if (packets < 1 || packets > sccsum::kWave) return SCCSUM_EINVAL;
    sccsum::t_knobs.tile_packets = packets;
    return SCCSUM_OK;
}

int sccsum_set_tile_bytes(int bytes) {
    if (bytes < 0) return SCCSUM_EINVAL;
    sccsum::t_knobs.tile_bytes = bytes;
    return SCCSUM_OK;
}

int sccsum_set_dynamic_tiles(int on) {
    if (on != 0 && on != 1) return SCCSUM_EINVAL;
    sccsum::t_knobs.dynamic = on;
    return SCCSUM_OK;
}

int sccsum_set_out_policy(int policy) {
    if (policy < 0 || policy > 4) return SCCSUM_EINVAL;
    sccsum::t_knobs.out_policy = policy;
    return SCCSUM_OK;
}

int sccsum_set_engine_write_through(int on) {
    sccsum::t_knobs.engine_wt = on ? 1 : 0;
    return SCCSUM_OK;
}

int sccsum_set_engine_sync_every(int steps) {
    if (steps < -1 || steps > 65536) return SCCSUM_EINVAL;
    sccsum::t_knobs.engine_sync_every = steps;
    return SCCSUM_OK;
}

int sccsum_set_engine_idle_ms(int ms) {
    if (ms < 0 || ms > 3600000) return SCCSUM_EINVAL;
    sccsum::t_knobs.engine_idle_ms = ms;
    return SCCSUM_OK;
}

int sccsum_set_short_chunks(int on) {
    if (on != 0 && on != 1) return SCCSUM_EINVAL;
    sccsum::t_knobs.short_chunks = on;
    return SCCSUM_OK;
}

int sccsum_set_run_align(int units) {
    if (units != 1 && units != 4 && units != 8) return SCCSUM_EINVAL;
    sccsum::t_knobs.run_align = units;
    return SCCSUM_OK;
}

int sccsum_set_tail_split(int split, int quarters) {
    if (!(split == 1 || split == 2 || split == 4 || split == 8) || quarters < 0 || quarters > 64) return SCCSUM_EINVAL;
    sccsum::t_knobs.tail_split = split;
    sccsum::t_knobs.tail_quarters = quarters;
    return SCCSUM_OK;
}

int sccsum_sync(void* stream) { return static_cast<int>(hipStreamSynchronize(static_cast<hipStream_t>(stream))); }

#ifdef SCCSUM_AB_TIMELINE
// A/B builds only: the per-wave timeline of the last flat launch (4 u64 per wave).
int sccsum_ab_timeline(void* host, uint64_t bytes) {
    const uint64_t n = bytes < sizeof(sccsum::g_timeline) ? bytes : sizeof(sccsum::g_timeline);
    return static_cast<int>(hipMemcpyFromSymbol(host, HIP_SYMBOL(sccsum::g_timeline), n, 0, hipMemcpyDeviceToHost));
}
// and the per-wave counters of the last engine run (8 u64 per wave)
int sccsum_ab_engine_stats(void* host, uint64_t bytes) {
    const uint64_t n = bytes < sizeof(sccsum::g_engine_stats) ? bytes : sizeof(sccsum::g_engine_stats);
    return static_cast<int>(hipMemcpyFromSymbol(host, HIP_SYMBOL(sccsum::g_engine_stats), n, 0, hipMemcpyDeviceToHost));
}
// and the per-step group / XCD retire times of the last engine run (then cleared):
// kStepRec x 64 u64, then kStepRec x 8 x 2 u64
int sccsum_ab_step_times(void* host, uint64_t bytes) {
    const uint64_t a = sizeof(sccsum::g_step_grp), b = sizeof(sccsum::g_step_xcd);
    if (bytes < a + b) return SCCSUM_EINVAL;
    hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(sccsum::g_step_grp), a, 0, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpyFromSymbol(static_cast<char*>(host) + a, HIP_SYMBOL(sccsum::g_step_xcd), b, 0, hipMemcpyDeviceToHost);
    void* pa = nullptr;
    void* pb = nullptr;
    if (e == hipSuccess) e = hipGetSymbolAddress(&pa, HIP_SYMBOL(sccsum::g_step_grp));
    if (e == hipSuccess) e = hipGetSymbolAddress(&pb, HIP_SYMBOL(sccsum::g_step_xcd));
    if (e == hipSuccess) e = hipMemset(pa, 0, a);
    if (e == hipSuccess) e = hipMemset(pb, 0, b);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return static_cast<int>(e);
}
#endif

int sccsum_read_probe_blocks(void) { return sccsum::current_cu_count() * sccsum::kBlocksPerCU; }

int sccsum_read_probe(const void* d_src, uint64_t bytes, uint64_t* d_sink, void* stream) {
    if (!d_src || !d_sink || (bytes & 15u) || sccsum::misaligned(d_src, 16)) return SCCSUM_EINVAL;
    const sccsum::LaunchTarget T(stream);
    if (T.rc != SCCSUM_OK) return T.rc;
    const unsigned grid = static_cast<unsigned>(sccsum::cu_count(T.dev) * sccsum::kBlocksPerCU) & ~7u;
    return static_cast<int>(sccsum::launch_kernel(sccsum::read_probe_kernel, dim3(grid), dim3(sccsum::kBlock), 0, T.s,
                                                  static_cast<const sccsum::u32x4*>(d_src), bytes / 16, d_sink));
}

}  // extern "C"
