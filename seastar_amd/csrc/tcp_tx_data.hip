// tcp_tx_data.hip — the TCP transmit fast path on the GPU: every polled
// connection's unsent queue cut into the segments one trip through the
// reference's transmit chain makes of it (sccsum.h, "TCP transmit fast path";
// DESIGN.md §5.19).
//
// What it restates from the reference (paths relative to the reference tree):
//   tcb::get_packet's continuation       include/seastar/net/tcp.hh:2089-2111
//   tcb::can_send                        tcp.hh:515-549, the branches a tcb with
//                                        dupacks == 0 and no window probe takes
//   tcb::get_transmit_packet             tcp.hh:1578-1606
//   tcb::output_one's sequence fields    tcp.hh:1635-1645, the timer 1700-1710
//
// On that path the chain has a closed form in the connection's state and the
// length U of its queue: it sends T = min(window - used, U) bytes in segments of
// P = min(cwnd, L) bytes, or one empty segment when there is nothing to send.
// So nothing is scanned over segments: a segment's place in every output is its
// connection's base plus a function of its index k, and the number of (segment,
// buffer) pieces before it is k plus the buffers that begin inside (0, k P)
// off a multiple of P — a prefix count over the buffers.
//
// Plain dependent launches on the caller's stream, no block waiting on another
// one, no atomic, no payload byte moves:
//   scan_tile / scan_carry / scan_place   (array_scan.h) twice over the buffers: the 64-bit
//                exclusive scan G of the lengths (a queue's length and a
//                buffer's stream offset are differences of it), then the 32-bit
//                scan M of "begins off a segment cut", which needs G
//   conn_count   per connection: segments, layout bytes, pieces; tile totals
//   conn_scan    ONE block: the tiles scanned, the capacity prefix, d_total
//   conn_place   per connection: its bases and its run record
//   seg_emit     parallel over SEGMENTS, striding past a block cap: a segment
//                finds its connection by search in the staged segment bases and
//                writes d_off, d_len, d_out, d_seg_first and its descriptors
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "array_scan.h"
#include "host_launch.h"
#include "sccsum.h"
#include "wave_scan.h"
#include "wire.h"

namespace tcp_tx_data {

using array_scan::LoadLen;
using array_scan::scan_array;   // the exclusive scan of an array: tile / carry / place
using host_launch::Chain;
using host_launch::misaligned;
using host_launch::stream_ok;
using host_launch::Workspace;
using wave_scan::block_inclusive_scan;
using wire::tiles_of;

constexpr int kWave = 64;
constexpr int kBlock = 1024;                 // threads of the scan and connection kernels: one item each
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kTile = kBlock;
constexpr int kSegBlock = 256;
constexpr int kSegRounds = 4;                // round r of a tile is its segments [256 r, 256 r + 256)
constexpr uint32_t kSegTile = kSegBlock * kSegRounds;
constexpr uint32_t kSegStage = 2048;         // segment bases a tile searches in LDS
constexpr uint32_t kSegMaxBlocks = 1024;     // the grid strides over the tiles past this
constexpr uint32_t kHdrs = 40;               // tcp_hdr_len_min + ip_hdr_len_min
constexpr uint64_t kNeedClamp = uint64_t(1) << 43;  // a connection's layout bytes count as at most this
constexpr uint64_t kMaxBufs = uint64_t(1) << 31;

static_assert(sizeof(sccsum_tcp_snd) == 48 && sizeof(sccsum_tcp_snd_run) == 32 && sizeof(sccsum_tcp_out) == 24 &&
                  sizeof(sccsum_gather_desc) == 16,
              "layout");
static_assert(offsetof(sccsum_tcp_snd, cwnd) == 16 && offsetof(sccsum_tcp_snd, sport) == 24 &&
                  offsetof(sccsum_tcp_snd, mss) == 28 && offsetof(sccsum_tcp_snd, flags) == 32 &&
                  offsetof(sccsum_tcp_snd_run, flags) == 16 && offsetof(sccsum_tcp_snd_run, stop) == 17,
              "the kernels read and write the records as 16-byte words");

// ---------------------------------------------------------------- one connection

struct In {
    const uint4* snd;          // sccsum_tcp_snd as three 16-byte words
    const uint64_t* buf_src;
    const uint32_t* buf_len;
    const uint32_t* buf_first;
    const uint64_t* G;         // workspace: the exclusive scan of buf_len, nbuf + 1 entries
    uint32_t nconns;
    uint32_t nbuf;
    uint32_t seg_len;          // L before the min with the mss; the whole of it with TSO
    uint32_t headroom;
    uint32_t tso;
};

// The last j in [lo, hi) with at(j) <= x, given at(lo) <= x.
template <typename At, typename X>
__device__ __forceinline__ uint64_t last_le(At at, X x, uint64_t lo, uint64_t hi) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (at(mid) <= x) lo = mid; else hi = mid;
    }
    return lo;
}

struct Conn {
    uint32_t a, b;             // its buffers, inside [0, nbuf] whatever buf_first says
    uint64_t base, U;          // G[a]; the queue's bytes
    uint32_t next, flags;
    uint32_t T, P, segs;       // what the chain sends, in segments of P (the last one shorter); segs 0: not taken
    uint32_t stop;
};

__device__ __forceinline__ Conn eval_conn(const In& I, uint32_t c) {
    Conn r{};
    const uint4 w0 = I.snd[3 * uint64_t(c)], w1 = I.snd[3 * uint64_t(c) + 1], w2 = I.snd[3 * uint64_t(c) + 2];
    const uint32_t a = I.buf_first[c], b = I.buf_first[c + 1];
    r.a = a < I.nbuf ? a : I.nbuf;
    r.b = b < r.a ? r.a : b < I.nbuf ? b : I.nbuf;
    r.base = I.G[r.a];
    r.U = I.G[r.b] - r.base;
    r.next = w0.y;
    r.flags = w2.x & 0xFFu;
    if (!(r.flags & SCCSUM_TCP_SND_ELIGIBLE)) {
        r.stop = SCCSUM_TCP_STOP_INELIGIBLE;
        return r;
    }
    if (r.U > 0xFFFFFFFFull) {  // the reference's uint32_t unsent_len would have wrapped
        r.stop = SCCSUM_TCP_STOP_QUEUE;
        return r;
    }
    const uint32_t window = w0.w, used = w0.y - w0.z, cwnd = w1.x, mss = w1.w & 0xFFFFu;
    const uint32_t U = static_cast<uint32_t>(r.U);
    const uint32_t can = (window == 0 || used > window) ? 0u : (window - used < U ? window - used : U);
    const uint32_t L = I.tso ? I.seg_len : (I.seg_len < mss ? I.seg_len : mss);
    r.P = cwnd < L ? cwnd : L;
    r.T = r.P ? can : 0u;       // nothing leaves through segments of no bytes
    r.segs = r.T ? (r.T - 1u) / r.P + 1u : 1u;  // the first output_one() is unconditional: the pure ACK
    r.stop = r.T == r.U ? SCCSUM_TCP_STOP_END : SCCSUM_TCP_STOP_WINDOW;
    return r;
}

// Buffer j begins off a segment cut of its connection: it splits a segment in two.
struct LoadMark {
    In I;
    __device__ __forceinline__ uint32_t operator()(uint64_t j) const {
        if (I.buf_len[j] == 0) return 0;
        const uint32_t* const first = I.buf_first;
        if (first[0] > j) return 0;  // before the first queue
        const uint32_t c = static_cast<uint32_t>(last_le([&](uint64_t k) { return first[k]; }, j, 0, uint64_t(I.nconns) + 1));
        if (c >= I.nconns) return 0;  // behind the last queue
        const Conn r = eval_conn(I, c);
        if (r.segs == 0 || r.T == 0 || j < r.a || j >= r.b) return 0;
        const uint64_t o = I.G[j] - r.base;
        return o < r.T && static_cast<uint32_t>(o) % r.P != 0 ? 1u : 0u;
    }
};

// The pieces of the connection's stream bytes [0, x), 0 < x <= T, with x a
// multiple of P or T itself: one per segment begun, one more per buffer that
// begins inside (0, x) off a cut.
__device__ __forceinline__ uint64_t pieces_before(const In& I, const uint32_t* __restrict__ M, const Conn& r,
                                                  uint64_t x) {
    const uint64_t* const G = I.G;
    const uint64_t ja = last_le([&](uint64_t j) { return G[j]; }, r.base + x, r.a, r.b);
    const uint64_t jx = G[ja] < r.base + x ? ja + 1 : ja;  // the first buffer at or behind x; those between hold no byte
    return (x - 1) / r.P + 1 + (M[jx] - M[r.a]);
}

struct Ws {
    uint64_t* c_segs;          // per connection: its count, then (conn_place) its base
    uint64_t* c_bytes;
    uint64_t* c_pieces;
    uint64_t* t_segs;          // per tile of connections
    uint64_t* t_bytes;
    uint64_t* t_pieces;
    uint64_t* head;            // {segments, connections, layout bytes, pieces} emitted
    const uint32_t* M;         // the exclusive scan of LoadMark, nbuf + 1 entries
};

__global__ __launch_bounds__(kBlock) void conn_count(In I, Ws W) {
    __shared__ uint64_t part[kWaves];
    const uint32_t c = blockIdx.x * kTile + threadIdx.x;
    uint64_t segs = 0, bytes = 0, pieces = 0;
    if (c < I.nconns) {
        const Conn r = eval_conn(I, c);
        segs = r.segs;
        bytes = uint64_t(r.T) + uint64_t(I.headroom) * r.segs;
        if (bytes > kNeedClamp) bytes = kNeedClamp;
        if (r.segs && r.T) pieces = pieces_before(I, W.M, r, r.T);
        W.c_segs[c] = segs;
        W.c_bytes[c] = bytes;
        W.c_pieces[c] = pieces;
    }
    uint64_t ts, tb, tp;
    (void)block_inclusive_scan<kWaves>(segs, part, &ts);
    (void)block_inclusive_scan<kWaves>(bytes, part, &tb);
    (void)block_inclusive_scan<kWaves>(pieces, part, &tp);
    if (threadIdx.x == 0) {
        W.t_segs[blockIdx.x] = ts;
        W.t_bytes[blockIdx.x] = tb;
        W.t_pieces[blockIdx.x] = tp;
    }
}

// ONE block.  The sums only grow, so exactly one tile, and in it one
// connection, has what lies before it fitting the caps and itself not: the
// thread that holds it writes the cut, no other one does.
__global__ __launch_bounds__(kBlock) void conn_scan(In I, Ws W, uint64_t max_segs, uint64_t max_bytes,
                                                    uint32_t* __restrict__ d_seg_first, uint64_t* __restrict__ d_total) {
    __shared__ uint64_t part[kWaves];
    __shared__ uint64_t cut_tile;
    __shared__ uint64_t at_cut[4];
    const uint64_t ntiles = tiles_of(I.nconns, kTile);
    const auto fits = [&](uint64_t s, uint64_t b) { return s <= max_segs && b <= max_bytes; };
    if (threadIdx.x == 0) cut_tile = ~uint64_t(0);
    __syncthreads();
    uint64_t segs = 0, bytes = 0, pieces = 0;  // carried over the chunks of 1024 tiles
    for (uint64_t base = 0; base < ntiles; base += kBlock) {
        const uint64_t t = base + threadIdx.x;
        const bool live = t < ntiles;
        const uint64_t s = live ? W.t_segs[t] : 0, b = live ? W.t_bytes[t] : 0, p = live ? W.t_pieces[t] : 0;
        uint64_t ssum, bsum, psum;
        const uint64_t si = segs + block_inclusive_scan<kWaves>(s, part, &ssum);
        const uint64_t bi = bytes + block_inclusive_scan<kWaves>(b, part, &bsum);
        const uint64_t pi = pieces + block_inclusive_scan<kWaves>(p, part, &psum);
        if (live) {
            W.t_segs[t] = si - s;
            W.t_bytes[t] = bi - b;
            W.t_pieces[t] = pi - p;
            if (fits(si - s, bi - b) && !fits(si, bi)) cut_tile = t;
        }
        segs += ssum;
        bytes += bsum;
        pieces += psum;
    }
    __syncthreads();
    const uint64_t tc = cut_tile;
    if (tc != ~uint64_t(0)) {
        // the caps fall inside tile tc: its connections once more, on top of its bases
        const uint64_t c = tc * kTile + threadIdx.x;
        const bool live = c < I.nconns;
        const uint64_t s = live ? W.c_segs[c] : 0, b = live ? W.c_bytes[c] : 0, p = live ? W.c_pieces[c] : 0;
        uint64_t total;
        const uint64_t si = W.t_segs[tc] + block_inclusive_scan<kWaves>(s, part, &total);
        const uint64_t bi = W.t_bytes[tc] + block_inclusive_scan<kWaves>(b, part, &total);
        const uint64_t pi = W.t_pieces[tc] + block_inclusive_scan<kWaves>(p, part, &total);
        if (live && fits(si - s, bi - b) && !fits(si, bi)) {
            at_cut[0] = si - s;
            at_cut[1] = c;
            at_cut[2] = bi - b;
            at_cut[3] = pi - p;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool cut = tc != ~uint64_t(0);
        const uint64_t es = cut ? at_cut[0] : segs, ep = cut ? at_cut[3] : pieces;
        W.head[0] = es;
        W.head[1] = cut ? at_cut[1] : uint64_t(I.nconns);
        W.head[2] = cut ? at_cut[2] : bytes;
        W.head[3] = ep;
        d_total[0] = es;
        d_total[1] = W.head[2];
        d_total[2] = ep;
        d_total[3] = bytes;
        d_seg_first[es] = static_cast<uint32_t>(ep);  // the closing entry
    }
}

__global__ __launch_bounds__(kBlock) void conn_place(In I, Ws W, uint4* __restrict__ d_run) {
    __shared__ uint64_t part[kWaves];
    const uint32_t c = blockIdx.x * kTile + threadIdx.x;
    const bool live = c < I.nconns;
    const uint64_t s = live ? W.c_segs[c] : 0, b = live ? W.c_bytes[c] : 0, p = live ? W.c_pieces[c] : 0;
    uint64_t total;
    const uint64_t sx = W.t_segs[blockIdx.x] + block_inclusive_scan<kWaves>(s, part, &total) - s;
    const uint64_t bx = W.t_bytes[blockIdx.x] + block_inclusive_scan<kWaves>(b, part, &total) - b;
    const uint64_t px = W.t_pieces[blockIdx.x] + block_inclusive_scan<kWaves>(p, part, &total) - p;
    if (!live) return;
    const Conn r = eval_conn(I, c);
    if (c >= W.head[1]) {  // from the first connection that does not fit onward: nothing, the state as given
        W.c_segs[c] = W.head[0];
        W.c_bytes[c] = W.head[2];
        W.c_pieces[c] = W.head[3];
        d_run[2 * uint64_t(c)] = make_uint4(0, 0, static_cast<uint32_t>(W.head[0]), r.next);
        d_run[2 * uint64_t(c) + 1] = make_uint4(SCCSUM_TCP_STOP_CAPACITY << 8, 0, 0, 0);
        return;
    }
    W.c_segs[c] = sx;
    W.c_bytes[c] = bx;
    W.c_pieces[c] = px;
    // output_one arms the retransmit timer behind a segment with bytes when it is not running (tcp.hh:1700-1710)
    const uint32_t arm = r.T && !(r.flags & SCCSUM_TCP_SND_RTX_ARMED) ? SCCSUM_TCP_SND_RTX_ARM : 0u;
    d_run[2 * uint64_t(c)] = make_uint4(r.segs, r.T, static_cast<uint32_t>(sx), r.next + r.T);
    d_run[2 * uint64_t(c) + 1] = make_uint4(arm | (r.stop << 8), 0, 0, 0);
}

struct Out {
    uint64_t* off;
    uint32_t* len;
    uint32_t* out;             // sccsum_tcp_out as six 32-bit words: d_out is 4-byte aligned
    uint32_t* seg_first;
    uint2* desc;               // sccsum_gather_desc as two 8-byte words
    uint64_t desc_room;        // max_segs + nbuf
};

__global__ __launch_bounds__(kSegBlock) void seg_emit(In I, Ws W, Out O) {
    __shared__ uint64_t range[2];          // the connections of the tile's first and last segment
    __shared__ uint32_t staged[kSegStage]; // their segment bases, when they fit
    const uint64_t emitted = W.head[0], prefix = W.head[1];
    const uint64_t* const seg_base = W.c_segs;
    const auto global_base = [&](uint64_t c) { return seg_base[c]; };
    for (uint64_t f0 = uint64_t(blockIdx.x) * kSegTile; f0 < emitted; f0 += uint64_t(gridDim.x) * kSegTile) {
        const uint64_t last = (emitted - f0 < kSegTile ? emitted : f0 + kSegTile) - 1;
        __syncthreads();  // the last tile's readers are done with range and staged
        if (threadIdx.x == 0) range[0] = last_le(global_base, f0, 0, prefix);
        if (threadIdx.x == kWave) range[1] = last_le(global_base, last, 0, prefix);
        __syncthreads();
        // the tile's segments belong to connections lo .. hi - 1: at most 1024 that have segments, and the
        // ones without between them
        const uint64_t lo = range[0], hi = range[1] + 1;
        const bool in_lds = hi - lo <= kSegStage;
        if (in_lds) {
            for (uint32_t j = threadIdx.x; j < hi - lo; j += kSegBlock) staged[j] = static_cast<uint32_t>(seg_base[lo + j]);
        }
        __syncthreads();
        const auto staged_base = [&](uint64_t c) { return uint64_t(staged[c - lo]); };
#pragma unroll 1
        for (int round = 0; round < kSegRounds; ++round) {
            const uint64_t f = f0 + uint64_t(round) * kSegBlock + threadIdx.x;
            if (f > last) continue;
            const uint32_t c = static_cast<uint32_t>(in_lds ? last_le(staged_base, f, lo, hi) : last_le(global_base, f, lo, hi));
            const Conn r = eval_conn(I, c);
            const uint64_t k = f - seg_base[c];
            if (k >= r.segs) continue;  // never: k is below the connection's segment count
            const uint64_t s0 = k * r.P;                 // below T: 32 bits
            const uint32_t len = r.T ? (r.T - s0 < r.P ? r.T - static_cast<uint32_t>(s0) : r.P) : 0u;
            const uint64_t lay = W.c_bytes[c] + k * (uint64_t(r.P) + I.headroom) + I.headroom;  // those before are full
            const uint4 w0 = I.snd[3 * uint64_t(c)], w1 = I.snd[3 * uint64_t(c) + 1];
            O.off[f] = lay;
            O.len[f] = len;
            uint32_t* const o = O.out + 6 * f;
            o[0] = w0.x;
            o[1] = r.next + static_cast<uint32_t>(s0);
            o[2] = w1.y;
            o[3] = w1.z;
            o[4] = (w1.w >> 16) | (0x10u << 16) | (20u << 24);  // the header window, ACK alone, no options
            o[5] = w1.w & 0xFFFFu;
            uint64_t at = W.c_pieces[c] + (s0 ? pieces_before(I, W.M, r, s0) : 0u);
            O.seg_first[f] = static_cast<uint32_t>(at);
            if (!len) continue;
            // whole buffers while they fit, then the part of the next one (tcp.hh:1594-1603); a buffer
            // of no bytes is no piece
            const uint64_t* const G = I.G;
            uint64_t j = last_le([&](uint64_t x) { return G[x]; }, r.base + s0, r.a, r.b);
            uint64_t pos = s0;
            const uint64_t end = s0 + len;
            for (; pos < end && j < r.b; ++j) {
                const uint32_t bl = I.buf_len[j];
                if (bl == 0) continue;
                const uint64_t bo = G[j] - r.base;       // <= pos < bo + bl
                const uint64_t upto = bo + bl < end ? bo + bl : end;
                if (at < O.desc_room) {                  // always, with queues that do not overlap
                    const uint64_t src = I.buf_src[j] + (pos - bo);
                    O.desc[2 * at] = make_uint2(static_cast<uint32_t>(src), static_cast<uint32_t>(src >> 32));
                    O.desc[2 * at + 1] = make_uint2(static_cast<uint32_t>(lay + (pos - s0)), static_cast<uint32_t>(upto - pos));
                }
                pos = upto;
                ++at;
            }
        }
    }
}

// ---------------------------------------------------------------- host side

constexpr uint32_t kKnownFlags = SCCSUM_TCP_TSO;

inline bool opts_ok(const sccsum_tcp_tx_opts& o) {
    if (o.mtu < 68 || o.mtu > 65535 || o.headroom < 20 || o.headroom > 65535 || (o.flags & ~kKnownFlags)) return false;
    return !(o.flags & SCCSUM_TCP_TSO) || (o.max_packet_len > kHdrs && o.max_packet_len <= 65535);
}

// The workspace: 8-byte things first.
struct Layout {
    uint64_t G, bt, c_segs, c_bytes, c_pieces, t_segs, t_bytes, t_pieces, head, M, mt, bytes;
};

Layout layout_of(uint64_t nconns, uint64_t nbuf) {
    Layout L{};
    const uint64_t btiles = tiles_of(nbuf, kTile) + 1, ctiles = tiles_of(nconns, kTile) + 1;
    host_launch::Carver c;
    L.G = c.take(8 * (nbuf + 1));
    L.bt = c.take(8 * btiles);
    L.c_segs = c.take(8 * nconns);
    L.c_bytes = c.take(8 * nconns);
    L.c_pieces = c.take(8 * nconns);
    L.t_segs = c.take(8 * ctiles);
    L.t_bytes = c.take(8 * ctiles);
    L.t_pieces = c.take(8 * ctiles);
    L.head = c.take(32);
    L.M = c.take(4 * (nbuf + 1));
    L.mt = c.take(4 * btiles);
    L.bytes = c.end();
    return L;
}

}  // namespace tcp_tx_data

extern "C" {

int sccsum_tcp_tx_data_seg_tile(void) { return static_cast<int>(tcp_tx_data::kSegTile); }
int sccsum_tcp_tx_data_max_blocks(void) { return static_cast<int>(tcp_tx_data::kSegMaxBlocks); }

uint64_t sccsum_tcp_tx_data_workspace(uint32_t nconns, uint64_t nbuf) {
    return tcp_tx_data::layout_of(nconns, nbuf).bytes;
}

int sccsum_tcp_tx_data(const sccsum_tcp_tx_opts* opts, const sccsum_tcp_snd* d_snd, uint32_t nconns,
                       const uint64_t* d_buf_src, const uint32_t* d_buf_len, const uint32_t* d_buf_first, uint64_t nbuf,
                       uint64_t max_segs, uint64_t max_out_bytes, sccsum_tcp_snd_run* d_run, uint64_t* d_off,
                       uint32_t* d_len, sccsum_tcp_out* d_out, uint32_t* d_seg_first, sccsum_gather_desc* d_desc,
                       uint64_t* d_total, void* d_workspace, void* stream) {
    using namespace tcp_tx_data;
    if (!opts || !opts_ok(*opts)) return SCCSUM_EINVAL;
    if (nconns > SCCSUM_TCP_MAX_CONNS || nbuf > kMaxBufs || max_segs > 0x7FFFFFFFull || max_out_bytes > 0xFFFFFFFFull) {
        return SCCSUM_EINVAL;
    }
    if (!d_total || !d_seg_first || !d_workspace) return SCCSUM_EINVAL;
    if (misaligned(d_total, 8) || misaligned(d_seg_first, 4) || misaligned(d_workspace, 16)) return SCCSUM_EINVAL;
    if (nconns != 0) {
        if (!d_snd || !d_buf_first || !d_run) return SCCSUM_EINVAL;
        if (nbuf != 0 && (!d_buf_src || !d_buf_len)) return SCCSUM_EINVAL;
        if (max_segs != 0 && (!d_off || !d_len || !d_out || !d_desc)) return SCCSUM_EINVAL;
        if (misaligned(d_snd, 16) || misaligned(d_run, 16) || misaligned(d_buf_src, 8) || misaligned(d_buf_len, 4) ||
            misaligned(d_buf_first, 4) || misaligned(d_off, 8) || misaligned(d_len, 4) || misaligned(d_out, 4) ||
            misaligned(d_desc, 8)) {
            return SCCSUM_EINVAL;
        }
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, -1);
    if (rc != SCCSUM_OK) return rc;

    const Layout L = layout_of(nconns, nbuf);
    const Workspace ws(d_workspace);
    const bool tso = (opts->flags & SCCSUM_TCP_TSO) != 0;
    // uint16_t(mtu - 40), as tcp.hh:1590 casts it
    const uint32_t seg_len = tso ? opts->max_packet_len - kHdrs : (opts->mtu - kHdrs) & 0xFFFFu;
    const In I{reinterpret_cast<const uint4*>(d_snd), d_buf_src, d_buf_len, d_buf_first, ws.u64(L.G), nconns,
               static_cast<uint32_t>(nconns ? nbuf : 0), seg_len, opts->headroom, tso ? 1u : 0u};
    const Ws W{ws.u64(L.c_segs), ws.u64(L.c_bytes), ws.u64(L.c_pieces), ws.u64(L.t_segs), ws.u64(L.t_bytes),
               ws.u64(L.t_pieces), ws.u64(L.head), ws.u32(L.M)};
    const dim3 block(kBlock), ctiles(static_cast<unsigned>(tiles_of(nconns, kTile)));
    Chain c{st};
    if (nconns != 0) {
        c.e = scan_array<uint64_t>(st, LoadLen{d_buf_len}, I.nbuf, ws.u64(L.bt), ws.u64(L.G));
        if (c.ok()) c.e = scan_array<uint32_t>(st, LoadMark{I}, I.nbuf, ws.u32(L.mt), ws.u32(L.M));
        c.launch(conn_count, ctiles, block, 0, I, W);
    }
    c.launch(conn_scan, dim3(1), block, 0, I, W, max_segs, max_out_bytes, d_seg_first, d_total);
    if (nconns == 0) return c.rc();
    c.launch(conn_place, ctiles, block, 0, I, W, reinterpret_cast<uint4*>(d_run));
    if (max_segs == 0) return c.rc();
    const uint64_t blocks = std::min<uint64_t>(tiles_of(max_segs, kSegTile), kSegMaxBlocks);
    const Out O{d_off, d_len, reinterpret_cast<uint32_t*>(d_out), d_seg_first, reinterpret_cast<uint2*>(d_desc),
                max_segs + nbuf};
    c.launch(seg_emit, dim3(static_cast<unsigned>(blocks)), dim3(kSegBlock), 0, I, W, O);
    return c.rc();
}

}  // extern "C"
