// tcp_listen.hip — the passive open for a batch: what tcp::received does with a
// segment that has no tcb on a listening port, for bucket 1 of a finished
// sccsum_tcp_rx in arrival order (sccsum.h, "TCP passive open").
//
// What it restates from the reference (paths relative to the reference tree):
//   tcp::received, no tcb            include/seastar/net/tcp.hh:888-929
//   tcb::input_handle_listen_state   tcp.hh:1115-1141
//   tcb::init_from_options           tcp.hh:1079-1112
//   tcb::get_isn                     tcp.hh:2067-2086
//   tcp_option::parse / fill         src/net/tcp.cc:34-79, 81-138
//   tcp::respond_with_reset          tcp.hh:981-1023 (tcp_reset.h)
//
// Plain dependent launches on the caller's stream.  The bucket's size m is read
// on the device; every grid is sized by the caller's bound m_max.
//   clear_kernel     the hash table and the per-port run starts emptied; m, taken = m
//   key_kernel       position i's connid and flags -> the workspace
//   insert_kernel    every eligible position into the table: a slot holds the
//                    SMALLEST position of its connid (atomic min on that value;
//                    which slot a connid takes depends on arrival, the value
//                    does not, and no output's place comes from the table)
//   cand_kernel      candidate = the table's position is my own; the (port,
//                    position) pair of every candidate and the tile's counts of
//                    the port's low digit
//   two radix passes scan_rows_kernel, sort_scatter_kernel (stable), the
//                    candidates alone; sum_kernel = their number; sort_count_kernel
//   head_kernel      where each port's run starts in the sorted candidates
//   rank_kernel      rank = place inside the run; rank < d_space[port]: created
//   stop_kernel      taken = the smallest position whose connid has a created
//                    candidate before it (atomic min on that value)
//   class_kernel     d_class: the port is full at i iff its d_space[port]-th
//                    candidate lies before i
//   compact.h twice  the NEW and the RESET positions, stable
//   new_kernel       one lane per created connection: the options parsed, the ISN's
//                    two MD5 blocks in registers, d_new, the SYN-ACK staging
//   reset_kernel     the answers; totals_kernel
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "bucket_pass.h"
#include "compact.h"
#include "host_launch.h"
#include "sccsum.h"
#include "tcp_reset.h"
#include "wave_scan.h"
#include "wire.h"

namespace tcp_listen {

using bucket_pass::kDigits;
using bucket_pass::scan_rows_kernel;
using host_launch::Chain;
using host_launch::misaligned;
using host_launch::stream_ok;
using host_launch::Workspace;
using wave_scan::block_inclusive_scan;
using wire::be32_at;
using wire::tiles_of;

constexpr int kWave = 64;
constexpr int kBlock = 1024;                 // threads of every tile kernel: one position each
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kTile = kBlock;
constexpr int kFlatBlock = 256;
constexpr uint32_t kPorts = 65536;
constexpr uint32_t kTcpHdr = 20;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kSyn = 2u, kRst = 4u, kAck = 16u;
constexpr uint32_t kRcvWindow = 29200;       // get_default_receive_window_size (tcp.hh:418-422)
constexpr uint32_t kLocalWscale = 7;         // tcp.cc:56
constexpr uint32_t kCreated = 3u;            // mark: 1 a candidate, 3 a created one

static_assert(sizeof(sccsum_tcp_new) == 64 && sizeof(sccsum_tcp_listen_opts) == 76, "layout");

// the workspace's scalars
enum : uint32_t { kM = 0, kCands = 1, kTaken = 2, kNew = 3, kResets = 4, kScalars = 8 };

struct In {
    const uint8_t* bytes;
    uint64_t bytes_len;
    const uint64_t* off;
    uint64_t nbatch;
    const uint32_t* first;
    const uint32_t* order;
    const uint2* seg;       // sccsum_tcp_seg as four 8-byte words
    const uint32_t* src;
    const uint32_t* space;
    uint32_t m_max;
};

struct Ws {
    uint4* key;             // [m]: local_ip, foreign_ip, local_port << 16 | foreign_port, the flags byte
    uint2* kv0;             // [m]: (port, position) pairs, the sort's two buffers
    uint2* kv1;
    uint32_t* table;        // [mask + 1]: the smallest eligible position of a connid, kNone when empty
    uint32_t mask;
    uint32_t* port_start;   // [65536]: where the port's candidates start in the sorted pairs
    uint32_t* counts;       // [256][pitch]
    uint32_t* totals;       // [256]
    uint32_t pitch;
    uint32_t* mark;         // [m]
    uint32_t* new_pos;      // [m]: the NEW positions, then the RESET ones
    uint32_t* rst_pos;
    uint32_t* tc_new;       // one word per tile
    uint32_t* tc_rst;
    uint32_t* sc;           // [kScalars]
};

struct Out {
    uint8_t* cls;
    uint4* rec;             // sccsum_tcp_new as four 16-byte words
    uint32_t* synack;       // 32 bytes = eight words per slot
    uint64_t* sa_off;
    uint32_t* sa_len;
    uint32_t* sa_out;       // sccsum_tcp_out as six words
    uint32_t* rst;
    uint32_t* rst_dst;
    uint64_t* total;
};

__device__ __forceinline__ bool eligible(uint32_t flags) { return (flags & (kSyn | kRst | kAck)) == kSyn; }

__device__ __forceinline__ bool same_connid(const uint4& a, const uint4& b) {
    return a.x == b.x && a.y == b.y && a.z == b.z;
}

// ---------------------------------------------------------------- the connids and their first eligible segment

__global__ __launch_bounds__(kBlock) void clear_kernel(In I, Ws W) {
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g <= W.mask) W.table[g] = kNone;
    if (g < kPorts) W.port_start[g] = kNone;
    if (g == 0) {
        const uint32_t lo = I.first[1], hi = I.first[2];
        const uint32_t size = hi > lo ? hi - lo : 0u;
        const uint32_t m = size < I.m_max ? size : I.m_max;
        W.sc[kM] = m;
        W.sc[kTaken] = m;
        W.sc[kCands] = 0;
        W.sc[kNew] = 0;
        W.sc[kResets] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void key_kernel(In I, Ws W) {
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    if (i >= W.sc[kM]) return;
    const uint64_t p = uint64_t(I.first[1]) + i;
    const uint2 d = I.seg[4 * p + 3];
    const uint32_t sport = d.x >> 16, dport = d.y & 0xFFFFu, flags = (d.y >> 16) & 0xFFu;
    const uint64_t frame = I.order[p];
    uint32_t local = 0;
    if (frame < I.nbatch) {
        const uint64_t o = I.off[frame];
        if (o <= I.bytes_len && I.bytes_len - o >= wire::kIpHdrMin) local = be32_at(I.bytes + o + 16);
    }
    W.key[i] = make_uint4(local, I.src[p], (dport << 16) | sport, flags);
}

__global__ __launch_bounds__(kBlock) void insert_kernel(Ws W) {
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    const uint32_t m = W.sc[kM];
    if (i >= m) return;
    const uint4 k = W.key[i];
    if (!eligible(k.w)) return;
    // A slot never changes owner: it goes from empty to one connid once (the compare-and-swap) and from
    // then on holds positions of that connid only (the atomic min is issued only after the keys compared
    // equal).  So a probe that passes an occupied slot would pass it on every later visit too, two
    // segments of one connid cannot settle in two slots, and whichever position a reader finds in a
    // slot names the slot's connid.  That rests on key_kernel having finished in the launch before (the
    // keys read here are complete) and on find() reading any value >= m, kNone included, as empty.
    uint32_t s = wire::connid_hash(k.x, k.y, k.z) & W.mask;
    for (uint32_t n = 0; n <= W.mask; ++n) {  // at most half of the slots are ever taken
        uint32_t cur = __hip_atomic_load(&W.table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kNone) {
            cur = atomicCAS(&W.table[s], kNone, i);
            if (cur == kNone) return;         // the slot is this connid's from now on
        }
        // whatever position stands here, it is one of the slot's connid: the keys are the last launch's
        if (cur < m && same_connid(W.key[cur], k)) {
            atomicMin(&W.table[s], i);
            return;
        }
        s = (s + 1u) & W.mask;
    }
}

// The smallest eligible position of the connid, or kNone.  After insert_kernel.
__device__ __forceinline__ uint32_t find(const Ws& W, const uint4& k, uint32_t m) {
    uint32_t s = wire::connid_hash(k.x, k.y, k.z) & W.mask;
    for (uint32_t n = 0; n <= W.mask; ++n) {
        const uint32_t cur = W.table[s];
        if (cur >= m) return kNone;           // empty
        if (same_connid(W.key[cur], k)) return cur;
        s = (s + 1u) & W.mask;
    }
    return kNone;
}

__global__ __launch_bounds__(kBlock) void cand_kernel(Ws W) {
    __shared__ uint32_t hist[kDigits];
    bucket_pass::hist_clear(hist);
    __syncthreads();
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    const uint32_t m = W.sc[kM];
    bool cand = false;
    uint32_t port = 0;
    if (i < m) {
        const uint4 k = W.key[i];
        port = k.z >> 16;
        cand = eligible(k.w) && find(W, k, m) == i;
        W.mark[i] = cand ? 1u : 0u;
        W.kv0[i] = make_uint2(cand ? port : kNone, i);
    }
    bucket_pass::hist_add(hist, port & 0xFFu, cand);
    __syncthreads();
    bucket_pass::hist_store(hist, kDigits, W.counts, W.pitch);
}

// ---------------------------------------------------------------- the candidates sorted by port

// The pairs [0, *n) of kv whose key is not kNone take part.
__global__ __launch_bounds__(kBlock) void sort_count_kernel(const uint2* __restrict__ kv, const uint32_t* __restrict__ n,
                                                            int shift, uint32_t* __restrict__ counts, uint32_t pitch) {
    __shared__ uint32_t hist[kDigits];
    bucket_pass::hist_clear(hist);
    __syncthreads();
    const uint32_t p = blockIdx.x * kTile + threadIdx.x;
    const uint32_t key = p < *n ? kv[p].x : kNone;
    bucket_pass::hist_add(hist, (key >> shift) & 0xFFu, key != kNone);
    __syncthreads();
    bucket_pass::hist_store(hist, kDigits, counts, pitch);
}

// Stable, as tcp.hip's: a pair's place is its digit's base, the pairs of the
// digit in the tiles before, and its offset among them inside the tile.
__global__ __launch_bounds__(kBlock) void sort_scatter_kernel(const uint2* __restrict__ kv, const uint32_t* __restrict__ n,
                                                              int shift, const uint32_t* __restrict__ counts,
                                                              uint32_t pitch, const uint32_t* __restrict__ totals,
                                                              uint2* __restrict__ kv_out, uint32_t room) {
    __shared__ uint32_t base[kDigits];
    __shared__ uint32_t part[kWaves];
    bucket_pass::TileRank<kWaves, 1, kDigits> rank;
    bucket_pass::digit_base<kWaves>(base, totals, counts, pitch, part);
    rank.clear(kDigits);
    __syncthreads();
    const uint32_t p = blockIdx.x * kTile + threadIdx.x;
    const uint2 e = p < *n ? kv[p] : make_uint2(kNone, 0);
    const bool valid = e.x != kNone;
    const uint32_t d = (e.x >> shift) & 0xFFu;
    rank.mark(0, d, valid);
    __syncthreads();
    rank.scan(kDigits);
    __syncthreads();
    if (!valid) return;
    const uint64_t pos = uint64_t(base[d]) + rank.offset(0, d);
    if (pos < room) kv_out[pos] = e;  // always true: the counts are this pass's own
}

// ONE block of 256 threads: the number of candidates is the sum of the first pass's digit totals.
__global__ __launch_bounds__(kFlatBlock) void sum_kernel(const uint32_t* __restrict__ totals, uint32_t* __restrict__ sc) {
    __shared__ uint32_t part[kFlatBlock / kWave];
    uint32_t all;
    (void)block_inclusive_scan<kFlatBlock / kWave>(totals[threadIdx.x], part, &all);
    if (threadIdx.x == 0) sc[kCands] = all;
}

__global__ __launch_bounds__(kBlock) void head_kernel(Ws W) {
    const uint32_t q = blockIdx.x * kTile + threadIdx.x;
    if (q >= W.sc[kCands]) return;
    const uint32_t port = W.kv0[q].x;
    if (port < kPorts && (q == 0 || W.kv0[q - 1].x != port)) W.port_start[port] = q;
}

__global__ __launch_bounds__(kBlock) void rank_kernel(In I, Ws W) {
    const uint32_t q = blockIdx.x * kTile + threadIdx.x;
    if (q >= W.sc[kCands]) return;
    const uint2 e = W.kv0[q];
    if (e.x >= kPorts || e.y >= W.sc[kM]) return;
    const uint32_t rank = q - W.port_start[e.x];
    if (rank < I.space[e.x]) W.mark[e.y] = kCreated;
}

// ---------------------------------------------------------------- the stop and the classes

__global__ __launch_bounds__(kBlock) void stop_kernel(Ws W) {
    __shared__ uint32_t best;
    if (threadIdx.x == 0) best = kNone;
    __syncthreads();
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    const uint32_t m = W.sc[kM];
    if (i < m) {
        const uint32_t c = find(W, W.key[i], m);
        if (c < i && W.mark[c] == kCreated) atomicMin(&best, i);  // LDS: only the minimum comes out
    }
    __syncthreads();
    if (threadIdx.x == 0 && best != kNone) atomicMin(&W.sc[kTaken], best);
}

// listener->full() as position i meets it: the port's d_space-th candidate lies before i.
__device__ __forceinline__ bool full_at(const In& I, const Ws& W, uint32_t port, uint32_t i) {
    const uint32_t space = I.space[port];
    if (space == 0) return true;
    const uint32_t start = W.port_start[port];
    if (start == kNone) return false;
    const uint64_t q = uint64_t(start) + space - 1u;
    if (q >= W.sc[kCands]) return false;
    const uint2 e = W.kv0[q];
    return e.x == port && e.y < i;
}

__global__ __launch_bounds__(kBlock) void class_kernel(In I, Ws W, uint8_t* __restrict__ cls) {
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    if (i >= W.sc[kM]) return;
    uint32_t c = SCCSUM_TCP_LISTEN_LATER;
    if (i < W.sc[kTaken]) {
        const uint4 k = W.key[i];
        const uint32_t flags = k.w;
        if (full_at(I, W, k.z >> 16, i)) {
            c = (flags & kRst) ? SCCSUM_TCP_LISTEN_DROP : SCCSUM_TCP_LISTEN_RESET;   // tcp.hh:890-898, 983-985
        } else if (flags & kRst) {
            c = SCCSUM_TCP_LISTEN_DROP;                                              // tcp.hh:902-905
        } else if (flags & kAck) {
            c = SCCSUM_TCP_LISTEN_RESET;                                             // tcp.hh:907-912
        } else if (flags & kSyn) {
            // before `taken` and not full: its connid's candidate, and its rank is below d_space
            c = SCCSUM_TCP_LISTEN_NEW;
        } else {
            c = SCCSUM_TCP_LISTEN_DROP;                                              // tcp.hh:925-928
        }
    }
    cls[i] = static_cast<uint8_t>(c);
}

// compact.h's predicate: the positions of one class.
struct OfClass {
    using Record = uint32_t;
    using Out = uint32_t;
    const uint8_t* cls;
    const uint32_t* sc;
    uint32_t want;
    __device__ __forceinline__ bool operator()(uint64_t i, Record* r) const {
        if (i >= sc[kM]) return false;
        *r = static_cast<uint32_t>(i);
        return cls[i] == want;
    }
    __device__ static __forceinline__ void store(Out* out, uint64_t pos, const Record& r) { out[pos] = r; }
};

// ---------------------------------------------------------------- a created connection

// MD5 (RFC 1321) of one 64-byte block given as sixteen little-endian words:
// fully unrolled, so the constants are immediates and the words stay in registers.
struct Md5 {
    uint32_t a, b, c, d;
};

__device__ __forceinline__ uint32_t rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }

__device__ __forceinline__ void md5_block(Md5& h, const uint32_t (&w)[16]) {
    constexpr uint32_t K[64] = {
        0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
        0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
        0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
        0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
        0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
        0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
        0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
        0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
    constexpr int S[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
    uint32_t a = h.a, b = h.b, c = h.c, d = h.d;
#pragma unroll
    for (int r = 0; r < 64; ++r) {
        uint32_t f;
        int g;
        if (r < 16) {
            f = (b & c) | (~b & d);
            g = r;
        } else if (r < 32) {
            f = (d & b) | (~d & c);
            g = (5 * r + 1) & 15;
        } else if (r < 48) {
            f = b ^ c ^ d;
            g = (3 * r + 5) & 15;
        } else {
            f = c ^ (b | ~d);
            g = (7 * r) & 15;
        }
        const uint32_t t = a + f + K[r] + w[g];
        a = d;
        d = c;
        c = b;
        b = b + rotl(t, S[(r >> 4) * 4 + (r & 3)]);
    }
    h.a += a;
    h.b += b;
    h.c += c;
    h.d += d;
}

// get_isn's digest word: MD5 of {local_ip, foreign_ip, ports} and the 64 key bytes, 76 bytes in two blocks.
__device__ __forceinline__ uint32_t isn_digest(uint32_t local_ip, uint32_t foreign_ip, uint32_t ports,
                                               const uint32_t (&key)[16]) {
    Md5 h{0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    uint32_t w[16];
    w[0] = local_ip;
    w[1] = foreign_ip;
    w[2] = ports;
#pragma unroll
    for (int k = 0; k < 13; ++k) w[3 + k] = key[k];
    md5_block(h, w);
    w[0] = key[13];
    w[1] = key[14];
    w[2] = key[15];
    w[3] = 0x80u;
#pragma unroll
    for (int k = 4; k < 16; ++k) w[k] = 0;
    w[14] = 76u * 8u;
    md5_block(h, w);
    return h.a;
}

// tcp_option::parse's state (tcp.hh:183-192).
struct Options {
    uint32_t mss = 536, shift = 0, flags = 0;
};

// tcp.cc:34-79 over o[0 .. len), byte loads only; it ends where the reference would read o[len] or beyond.
__device__ __forceinline__ Options parse(const uint8_t* __restrict__ o, uint32_t len) {
    Options opt;
    uint32_t at = 0;
    while (at < len) {
        const uint32_t kind = o[at];
        uint32_t size = 0;
        if (kind != 1u && kind != 0u) {
            if (at + 1u >= len) break;                 // the length byte is not there
            size = o[at + 1u];
            if (at + size > len) break;                // tcp.cc:42
        }
        if (kind == 2u) {
            if (at + 3u >= len) break;                 // the value is not there
            opt.flags |= SCCSUM_TCP_NEW_MSS;
            opt.mss = (uint32_t(o[at + 2u]) << 8) | o[at + 3u];
            at += 4u;
        } else if (kind == 3u) {
            if (at + 2u >= len) break;
            opt.flags |= SCCSUM_TCP_NEW_WSCALE;
            opt.shift = o[at + 2u];
            at += 3u;
        } else if (kind == 4u) {
            opt.flags |= SCCSUM_TCP_NEW_SACK;
            at += 2u;
        } else if (kind == 1u) {
            at += 1u;
        } else if (kind == 0u) {
            break;
        } else {
            if (size == 0) break;                      // tcp.cc:72-75
            at += size;
        }
    }
    return opt;
}

__global__ __launch_bounds__(kFlatBlock) void new_kernel(In I, Ws W, Out O, sccsum_tcp_listen_opts opts) {
    const uint32_t k = blockIdx.x * kFlatBlock + threadIdx.x;
    if (k >= W.sc[kNew]) return;
    const uint32_t i = W.new_pos[k];
    const uint4 id = W.key[i];
    const uint64_t p = uint64_t(I.first[1]) + i;
    const uint2 a = I.seg[4 * p], b = I.seg[4 * p + 1], c = I.seg[4 * p + 2], d = I.seg[4 * p + 3];
    const uint64_t pay_off = (uint64_t(a.y) << 32) | a.x;
    const uint32_t seq = b.y, ack = c.x, window = d.x & 0xFFFFu, hdr_len = d.y >> 24;
    uint32_t opt_len = hdr_len > kTcpHdr ? hdr_len - kTcpHdr : 0u;
    if (pay_off > I.bytes_len || pay_off < opt_len) opt_len = 0;
    const Options opt = parse(I.bytes + (pay_off - opt_len), opt_len);

    const uint32_t local_port = id.z >> 16, foreign_port = id.z & 0xFFFFu;
    const uint32_t iss = isn_digest(id.x, id.y, (local_port << 16) + foreign_port, opts.isn_key) + opts.isn_m;
    const uint32_t local_mss = (opts.mtu - 40u) & 0xFFFFu;
    const bool wscale = (opt.flags & SCCSUM_TCP_NEW_WSCALE) != 0, mss = (opt.flags & SCCSUM_TCP_NEW_MSS) != 0;
    const uint32_t rcv_wscale = wscale ? kLocalWscale : 0u;
    const bool big = opt.shift > 14u;
    const uint32_t snd_window = big ? window : window << opt.shift;
    const uint32_t cwnd = (opt.mss > 2190u ? 2u : opt.mss > 1095u ? 3u : 4u) * opt.mss;   // tcp.hh:1102-1108
    const uint32_t flags = opt.flags | (big ? SCCSUM_TCP_NEW_WSCALE_BIG : 0u);
    O.rec[4 * uint64_t(k)] = make_uint4(id.x, id.y, local_port | (foreign_port << 16), i);
    O.rec[4 * uint64_t(k) + 1] = make_uint4(seq, iss, snd_window, cwnd);
    O.rec[4 * uint64_t(k) + 2] = make_uint4(snd_window, kRcvWindow << rcv_wscale, seq, ack);
    O.rec[4 * uint64_t(k) + 3] = make_uint4(opt.mss | (local_mss << 16), opt.shift | (rcv_wscale << 8) | (flags << 16), 0, 0);

    // tcp_option::fill for SYN|ACK (tcp.cc:81-116): MSS, window scale, NOPs up to the EOL that ends a 4-byte group
    uint32_t w5 = 0, w6 = 0, hdr = kTcpHdr;
    const uint32_t mss_opt = 0x0402u | ((local_mss >> 8) << 16) | ((local_mss & 0xFFu) << 24);
    const uint32_t ws_opt = 0x0303u | (kLocalWscale << 16);                               // and the EOL
    if (mss && wscale) {
        w5 = mss_opt;
        w6 = ws_opt;
        hdr = 28;
    } else if (mss) {
        w5 = mss_opt;
        w6 = 0x00010101u;                                                                 // NOP NOP NOP EOL
        hdr = 28;
    } else if (wscale) {
        w5 = ws_opt;
        hdr = 24;
    }
    uint32_t* const slot = O.synack + 8 * uint64_t(k);   // the twenty bytes in front are sccsum_tcp_send's
    slot[5] = w5;
    slot[6] = w6;
    slot[7] = 0;
    O.sa_off[k] = 32 * uint64_t(k) + hdr;
    O.sa_len[k] = 0;
    uint32_t* const out = O.sa_out + 6 * uint64_t(k);
    out[0] = id.y;
    out[1] = iss;
    out[2] = seq + 1u;
    out[3] = local_port | (foreign_port << 16);
    out[4] = kRcvWindow | ((kSyn | kAck) << 16) | (hdr << 24);
    out[5] = opt.mss;
}

__global__ __launch_bounds__(kFlatBlock) void reset_kernel(In I, Ws W, Out O, uint32_t flags) {
    const uint32_t r = blockIdx.x * kFlatBlock + threadIdx.x;
    if (r >= W.sc[kResets]) return;
    const uint32_t i = W.rst_pos[r];
    const uint4 id = W.key[i];
    const uint64_t p = uint64_t(I.first[1]) + i;
    tcp_reset::answer(I.seg[4 * p + 1].y, I.seg[4 * p + 2].x, id.z & 0xFFFFu, id.z >> 16, id.w, id.y, id.x, flags,
                      O.rst + 5 * uint64_t(r), O.rst_dst + r);
}

__global__ void totals_kernel(const uint32_t* __restrict__ sc, uint64_t* __restrict__ total) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint64_t taken = sc ? sc[kTaken] : 0u, created = sc ? sc[kNew] : 0u, resets = sc ? sc[kResets] : 0u;
    total[0] = taken;
    total[1] = created;
    total[2] = resets;
    total[3] = taken - created - resets;
}

// ---------------------------------------------------------------- host side

uint32_t slot_bits(uint64_t m_max) {
    uint32_t bits = 4;
    while ((uint64_t(1) << bits) < 2 * m_max) ++bits;
    return bits;
}

// The workspace: 16-byte things first, then 8, then 4.
struct Layout {
    uint64_t key, kv0, kv1, table, port_start, counts, totals, mark, new_pos, rst_pos, tc_new, tc_rst, sc, bytes;
    uint32_t ntiles, pitch, bits;
};

Layout layout_of(uint64_t m) {
    Layout L{};
    L.ntiles = static_cast<uint32_t>(tiles_of(m, kTile));
    L.pitch = bucket_pass::pitch_of(L.ntiles);
    L.bits = slot_bits(m);
    host_launch::Carver c;
    L.key = c.take(16 * m, 16);
    L.kv0 = c.take(8 * m, 16);
    L.kv1 = c.take(8 * m, 16);
    L.counts = c.take(uint64_t(kDigits) * L.pitch * 4u, 16);
    L.table = c.take(4 * (uint64_t(1) << L.bits), 16);
    L.port_start = c.take(4 * uint64_t(kPorts), 16);
    L.totals = c.take(4 * uint64_t(kDigits), 16);
    L.mark = c.take(4 * m, 16);
    L.new_pos = c.take(4 * m, 16);
    L.rst_pos = c.take(4 * m, 16);
    L.tc_new = c.take(4 * (uint64_t(L.ntiles) + 4u), 16);
    L.tc_rst = c.take(4 * (uint64_t(L.ntiles) + 4u), 16);
    L.sc = c.take(4 * uint64_t(kScalars), 16);
    L.bytes = c.end();
    return L;
}

}  // namespace tcp_listen

extern "C" {

uint64_t sccsum_tcp_listen_workspace(uint64_t m_max) {
    if (m_max > SCCSUM_TCP_LISTEN_MAX) return 0;
    return tcp_listen::layout_of(m_max).bytes;
}

int sccsum_tcp_listen(sccsum_tcp_listen_opts opts, const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off,
                      uint64_t nbatch, const uint32_t* d_first, const uint32_t* d_order, const sccsum_tcp_seg* d_seg,
                      const uint32_t* d_src, uint64_t m_max, const uint32_t* d_space, uint8_t* d_class,
                      sccsum_tcp_new* d_new, void* d_synack, uint64_t* d_sa_off, uint32_t* d_sa_len,
                      sccsum_tcp_out* d_sa_out, void* d_rst, uint32_t* d_rst_dst, uint64_t* d_total, void* d_workspace,
                      void* stream) {
    using namespace tcp_listen;
    if (opts.mtu < 68 || opts.mtu > 65535) return SCCSUM_EINVAL;
    if (opts.flags & ~uint32_t(SCCSUM_TCP_CSUM_OFFLOAD)) return SCCSUM_EINVAL;
    if (m_max > SCCSUM_TCP_LISTEN_MAX || nbatch > 0xFFFFFFFFull) return SCCSUM_EINVAL;
    if (!d_total || !d_workspace || misaligned(d_total, 8) || misaligned(d_workspace, 16)) return SCCSUM_EINVAL;
    if (m_max != 0) {
        if (!d_first || !d_order || !d_seg || !d_src || !d_space || !d_class || !d_new || !d_synack || !d_sa_off ||
            !d_sa_len || !d_sa_out || !d_rst || !d_rst_dst) {
            return SCCSUM_EINVAL;
        }
        if ((!d_bytes && bytes_len != 0) || (!d_off && nbatch != 0)) return SCCSUM_EINVAL;
        if (misaligned(d_off, 8) || misaligned(d_first, 4) || misaligned(d_order, 4) || misaligned(d_seg, 8) ||
            misaligned(d_src, 4) || misaligned(d_space, 4) || misaligned(d_new, 16) || misaligned(d_synack, 4) ||
            misaligned(d_sa_off, 8) || misaligned(d_sa_len, 4) || misaligned(d_sa_out, 4) || misaligned(d_rst, 4) ||
            misaligned(d_rst_dst, 4)) {
            return SCCSUM_EINVAL;
        }
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, -1);
    if (rc != SCCSUM_OK) return rc;
    Chain c{st};
    if (m_max == 0) {
        c.launch(totals_kernel, dim3(1), dim3(kWave), 0, nullptr, d_total);
        return c.rc();
    }

    const Layout L = layout_of(m_max);
    const Workspace ws(d_workspace);
    const uint32_t m = static_cast<uint32_t>(m_max);
    const In I{static_cast<const uint8_t*>(d_bytes), bytes_len, d_off, nbatch, d_first, d_order,
               reinterpret_cast<const uint2*>(d_seg), d_src, d_space, m};
    const Ws W{ws.at<uint4>(L.key), ws.at<uint2>(L.kv0), ws.at<uint2>(L.kv1), ws.u32(L.table),
               static_cast<uint32_t>((uint64_t(1) << L.bits) - 1u), ws.u32(L.port_start), ws.u32(L.counts),
               ws.u32(L.totals), L.pitch, ws.u32(L.mark), ws.u32(L.new_pos), ws.u32(L.rst_pos), ws.u32(L.tc_new),
               ws.u32(L.tc_rst), ws.u32(L.sc)};
    const Out O{d_class, reinterpret_cast<uint4*>(d_new), static_cast<uint32_t*>(d_synack), d_sa_off, d_sa_len,
                reinterpret_cast<uint32_t*>(d_sa_out), static_cast<uint32_t*>(d_rst), d_rst_dst, d_total};
    const dim3 tiles(L.ntiles), block(kBlock), rows(kDigits), wave(kWave);
    const uint64_t slots = uint64_t(1) << L.bits;
    const dim3 clear_grid(static_cast<unsigned>(tiles_of(slots > kPorts ? slots : kPorts, kBlock)));
    const dim3 flat(static_cast<unsigned>(tiles_of(m_max, kFlatBlock))), flat_block(kFlatBlock);
    const uint32_t* const n_all = W.sc + kM;
    const uint32_t* const n_cands = W.sc + kCands;

    c.launch(clear_kernel, clear_grid, block, 0, I, W);
    c.launch(key_kernel, tiles, block, 0, I, W);
    c.launch(insert_kernel, tiles, block, 0, W);
    c.launch(cand_kernel, tiles, block, 0, W);
    // the candidates by port: two stable 8-bit passes, kv0 -> kv1 -> kv0
    c.launch(scan_rows_kernel<>, rows, wave, 0, W.counts, L.ntiles, L.pitch, W.totals);
    c.launch(sum_kernel, dim3(1), flat_block, 0, W.totals, W.sc);
    c.launch(sort_scatter_kernel, tiles, block, 0, W.kv0, n_all, 0, W.counts, L.pitch, W.totals, W.kv1, m);
    c.launch(sort_count_kernel, tiles, block, 0, W.kv1, n_cands, 8, W.counts, L.pitch);
    c.launch(scan_rows_kernel<>, rows, wave, 0, W.counts, L.ntiles, L.pitch, W.totals);
    c.launch(sort_scatter_kernel, tiles, block, 0, W.kv1, n_cands, 8, W.counts, L.pitch, W.totals, W.kv0, m);
    c.launch(head_kernel, tiles, block, 0, W);
    c.launch(rank_kernel, tiles, block, 0, I, W);
    c.launch(stop_kernel, tiles, block, 0, W);
    c.launch(class_kernel, tiles, block, 0, I, W, d_class);
    if (c.ok()) {
        c.e = compact::run<kBlock>(st, OfClass{d_class, W.sc, SCCSUM_TCP_LISTEN_NEW}, L.ntiles, W.tc_new, W.sc + kNew,
                                   W.new_pos);
    }
    if (c.ok()) {
        c.e = compact::run<kBlock>(st, OfClass{d_class, W.sc, SCCSUM_TCP_LISTEN_RESET}, L.ntiles, W.tc_rst,
                                   W.sc + kResets, W.rst_pos);
    }
    c.launch(new_kernel, flat, flat_block, 0, I, W, O, opts);
    c.launch(reset_kernel, flat, flat_block, 0, I, W, O, opts.flags);
    c.launch(totals_kernel, dim3(1), wave, 0, W.sc, d_total);
    return c.rc();
}

}  // extern "C"
