// tcp_reset.h — the answer of tcp::respond_with_reset
// (include/seastar/net/tcp.hh:981-1023) to one segment, as tcp.hip writes it
// for the segments nobody owns and tcp_listen.hip for those a listener refuses
// (sccsum.h, "TCP layer": d_rst, d_rst_dst).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sccsum.h"
#include "wire.h"

namespace tcp_reset {

// The segment's header words as sccsum_tcp_seg holds them: seq, ack, sport,
// dport, flags.  src is the foreign address, dst ours.  out: the answer's five
// 32-bit words, 4-byte aligned; *out_dst: where it goes.
__device__ __forceinline__ void answer(uint32_t in_seq, uint32_t in_ack, uint32_t in_sport, uint32_t in_dport,
                                       uint32_t in_flags, uint32_t src, uint32_t dst, uint32_t flags,
                                       uint32_t* __restrict__ out, uint32_t* __restrict__ out_dst) {
    constexpr uint32_t kRst = 4u, kSyn = 2u, kAck = 16u, kTcpHdr = 20u, kProtoTcp = 6u;
    const uint32_t seq = (in_flags & kAck) ? in_ack : 0u;
    const bool syn = (in_flags & kSyn) != 0;
    const uint32_t ack = syn ? in_seq + 1u : 0u;
    const uint32_t fl = kRst | (syn ? kAck : 0u);
    const uint32_t w3 = ((kTcpHdr / 4u) << 28) | (fl << 16);   // data_offset, flags, window 0
    const uint32_t seed = wire::pseudo_seed(dst, src, kProtoTcp, kTcpHdr);
    uint32_t field;
    if (flags & SCCSUM_TCP_CSUM_OFFLOAD) {
        field = seed;                                          // ~csum.get(): the folded sum itself
    } else {
        const uint64_t s = uint64_t(seed) + in_dport + in_sport + (seq >> 16) + (seq & 0xFFFFu) + (ack >> 16) +
                           (ack & 0xFFFFu) + (w3 >> 16);
        field = 0xFFFFu ^ wire::fold16(s);
    }
    out[0] = __builtin_bswap32((in_dport << 16) | in_sport);   // the ports swapped
    out[1] = __builtin_bswap32(seq);
    out[2] = __builtin_bswap32(ack);
    out[3] = __builtin_bswap32(w3);
    out[4] = __builtin_bswap32(field << 16);                   // urgent 0
    *out_dst = src;
}

}  // namespace tcp_reset
