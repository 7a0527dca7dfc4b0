// wire.h — what every layer reads of a packet and of a call the same way: the
// big-endian fields, the folded pseudo-header sum, murmur3's finalizer, the
// caller's status masks, the tiles of a batch, and the common start of the
// IPv4 acceptance test (reasm.hip, udp.hip, tcp.hip; eth.hip and send.hip
// take the small pieces).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace wire {

constexpr int kMaxDevices = 64;
constexpr uint32_t kIpHdrMin = 20;

__host__ __device__ inline uint64_t tiles_of(uint64_t n, uint32_t tile) { return (n + tile - 1) / tile; }

__device__ __forceinline__ uint32_t be16_at(const uint8_t* p) { return (uint32_t(p[0]) << 8) | p[1]; }
__device__ __forceinline__ uint32_t be32_at(const uint8_t* p) {
    return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3];
}

__host__ __device__ inline uint32_t fold16(uint64_t s) {
    while (s >> 16) s = (s & 0xFFFFu) + (s >> 16);
    return static_cast<uint32_t>(s);
}

// ipv4_traits::{udp,tcp}_pseudo_header_checksum folded, as sccsum_pseudo_seed (ip.hh:70-75).
__host__ __device__ inline uint32_t pseudo_seed(uint32_t src, uint32_t dst, uint32_t proto, uint32_t len16) {
    return fold16(uint64_t(src) + dst + proto + len16);
}

__host__ __device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// The home slot of a TCP connid {local_ip, foreign_ip, local_port << 16 |
// foreign_port}: the three words mixed, then murmur3's finalizer
// (sccsum_tcp_conns_slot).
__host__ __device__ inline uint32_t connid_hash(uint32_t local_ip, uint32_t foreign_ip, uint32_t ports) {
    uint32_t h = local_ip * 0x9E3779B1u;
    h = (h ^ foreign_ip) * 0x85EBCA6Bu;
    return fmix32(h ^ ports);
}

// The caller's status masks: every bit of `need`, none of `reject`.
__device__ __forceinline__ bool status_passes(uint32_t st, uint32_t need, uint32_t reject) {
    return (st & need) == need && (st & reject) == 0;
}

// An IPv4 header that ipv4_view has accepted: its twenty fixed bytes lie
// inside the buffer, so every field may be read.
struct Ipv4View {
    const uint8_t* h;
    uint32_t hdr_len, ip_len, frag;  // frag: the flags and the fragment offset, bytes 6-7
    __device__ __forceinline__ uint32_t id() const { return be16_at(h + 4); }
    __device__ __forceinline__ uint32_t proto() const { return h[9]; }
    __device__ __forceinline__ uint32_t src() const { return be32_at(h + 12); }
    __device__ __forceinline__ uint32_t dst() const { return be32_at(h + 16); }
};

// The tests of ip.cc:128-144 that every rx layer repeats on the header itself,
// each before anything behind it is read: the frame inside the buffer, twenty
// bytes of it, then the header's own two lengths against the frame's.  The
// fragment word is loaded with the lengths, not behind the test on them: the
// layers test it next, and a load that waits for that branch is one more
// memory round trip per frame.  A refused frame's view is all zeros.
__device__ __forceinline__ bool ipv4_view(const uint8_t* bytes, uint64_t bytes_len, uint64_t off, uint32_t len,
                                          Ipv4View* v) {
    *v = Ipv4View{nullptr, 0, 0, 0};
    if (off > bytes_len || len > bytes_len - off || len < kIpHdrMin) return false;
    v->h = bytes + off;
    v->hdr_len = 4u * (v->h[0] & 0xFu);
    v->ip_len = be16_at(v->h + 2);
    v->frag = be16_at(v->h + 6);
    return !(len < v->ip_len || v->hdr_len > v->ip_len);
}

}  // namespace wire
