// tcp_data.hip — the TCP receive fast path on the GPU: the leading in-sequence
// stretch of every connection's run of sccsum_tcp_rx's bucket 0 (sccsum.h,
// "TCP receive fast path").
//
// What it restates from the reference (paths relative to the reference tree):
//   tcb::segment_acceptable              include/seastar/net/tcp.hh:1058-1076
//   tcb::input_handle_other_state        tcp.hh:1215-1575, of which only step
//                                        4.7 (tcp.hh:1497-1521) does anything
//                                        on the straight path
//   get_modified_receive_window_size     tcp.hh:424-427
//   tcb::should_send_ack                 tcp.hh:1845-1872
//
// Segment i of a run is taken iff every earlier one was and it passes the
// stops of sccsum.h.  While all earlier segments are taken the running state
// is a function of S_i, the sum of the pay_len of the run's segments before i,
// so "passes" is computed for every segment from S_i alone and the first one
// that does not pass ends the stretch: a segmented scan.  The delayed-ACK rule
// is a 4-state transducer ({nr_full} x {armed}); a segment's step is a table
// of four 4-bit entries and tables compose, so it rides in the same scan.
//
// Plain dependent launches on the caller's stream, one tile of kTile records
// per block, no block waiting on another one and no atomic at all:
//   sum_tile     per record: pay_len and the transducer table, scanned per run
//                inside the tile; the tile's open-run aggregate and head count
//   sum_carry    one block: the aggregates scanned across tiles (segmented),
//                chunked: what the run entering each tile has summed so far
//   stop_tile    per record: S_i exact, so the stop is exact; the tile's taken
//                records and bytes before and after its first head, and whether
//                the run leaving it has stopped
//   stop_carry   one block: which runs enter their tile already stopped, the
//                taken records and bytes before every tile, the tile where
//                max_bytes is passed (the capacity cut), d_total
//   place        per record: the descriptor of every taken one (its index is
//                the number of taken records before it, so descriptors are
//                grouped by run in arrival order), the run records, written by
//                the first record that stops or the last one of the run
//   cut_runs     the runs from the cut onward get desc_first / dst_off
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "host_launch.h"
#include "sccsum.h"
#include "wave_scan.h"
#include "wire.h"

namespace tcp_data {

using host_launch::Chain;
using host_launch::misaligned;
using host_launch::stream_ok;
using host_launch::Workspace;
using wave_scan::block_inclusive_scan;
using wire::tiles_of;

constexpr int kWave = 64;
constexpr int kBlock = 1024;                 // threads of every tile kernel: one record each
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kTile = kBlock;
constexpr int kFlatBlock = 256;
constexpr uint32_t kClamp = 1u << 30;        // room and cap above it are read as it
constexpr uint32_t kIdent = 0x3210u;         // the table that leaves every state alone
constexpr uint32_t kHead = 1u << 16;         // Elem::meta: a run head at or before this record, in the tile
constexpr int kPosShift = 17;                // ... and that head's thread index

static_assert(sizeof(sccsum_tcp_rcv) == 32 && sizeof(sccsum_tcp_rcv_run) == 32 && sizeof(sccsum_gather_desc) == 16,
              "layout");

// ---------------------------------------------------------------- the delayed-ACK transducer

// State s = nr_full | armed << 1.  A table holds for each s four bits at 4 s:
// the next state, 4 = the timer was armed anew, 8 = should_send_ack returned
// true (clear_delayed_ack(); output()).  tcp.hh:1845-1872 literally, seg_len
// being a uint16_t there:
//   seg_len > mss   nr_full = 0, cancel, true                        every s -> 0 | 8
//   seg_len == mss  nr_full++ >= 1: nr_full = 0, cancel, true        s with nr_full -> 0 | 8
//                   else nr_full = 1 and the timer rule below
//   the timer rule  armed: nothing; else arm(200 ms)
__host__ __device__ inline uint32_t table_of(uint32_t pay_len, uint32_t mss) {
    const uint32_t len = pay_len & 0xFFFFu;
    return len > mss ? 0x8888u : len == mss ? 0x8387u : 0x3276u;
}

// First a, then b.
__host__ __device__ inline uint32_t compose(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t ea = (a >> (4 * s)) & 15u;
        const uint32_t eb = (b >> (4 * (ea & 3u))) & 15u;
        r |= ((eb & 3u) | ((ea | eb) & 12u)) << (4 * s);
    }
    return r;
}

// ---------------------------------------------------------------- scans

// What a run has summed up to a record: the text and the composed table.
struct Elem {
    uint64_t sum;
    uint32_t meta;  // the table | kHead | head position << kPosShift
};

struct SegSum {
    __device__ __forceinline__ Elem operator()(const Elem& a, const Elem& b) const {
        if (b.meta & kHead) return b;
        return Elem{a.sum + b.sum, (a.meta & ~0xFFFFu) | compose(a.meta & 0xFFFFu, b.meta & 0xFFFFu)};
    }
};

// A segmented count: bit 31 a head at or before, the low bits the count since.
struct SegCount {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const {
        return (b >> 31) ? b : a + b;
    }
};

__device__ __forceinline__ Elem shfl_up(const Elem& v, int d) {
    return Elem{wave_scan::shfl_up(v.sum, d), wave_scan::shfl_up(v.meta, d)};
}

// wave_scan's scan of an associative op over the block's 1024 threads.
template <typename T, typename Op>
__device__ __forceinline__ T block_scan(T v, const T& ident, T* part, T* total, Op op) {
    return wave_scan::block_scan<kWaves>(v, ident, part, total, op);
}

// ---------------------------------------------------------------- one record

struct In {
    const uint2* seg;        // sccsum_tcp_seg as four 8-byte words: d_seg is 8-byte aligned
    const uint32_t* first;   // d_first of sccsum_tcp_rx: bucket 0 is [0, first[1])
    const uint4* rcv;        // sccsum_tcp_rcv as two 16-byte words
    uint64_t n;
    uint32_t nconns;
};

// The workspace, per tile; the carries have one entry more.
struct Ws {
    uint64_t* agg_sum;       // sum_tile: the aggregate of the tile ...
    uint32_t* agg_meta;
    uint32_t* heads;         // ... and its run heads
    uint64_t* in_sum;        // sum_carry: what the run entering tile t has summed
    uint32_t* in_meta;
    uint32_t* heads_before;
    uint64_t* hbytes;        // stop_tile: taken before the tile's first head, unless the run came in stopped
    uint64_t* rbytes;        // ... and from it on
    uint32_t* hcnt;
    uint32_t* rcnt;
    uint32_t* tflags;        // 1 a stop before the first head, 2 a head, 4 the run leaving has stopped
    uint64_t* bytes_in;      // stop_carry: taken before tile t
    uint64_t* cnt_in;
    uint32_t* stopped_in;
    uint32_t* cut;           // {kind, position, tile, 0}
};

constexpr uint32_t kCutNone = 0, kCutAt = 1, kCutInTile = 2;

__device__ __forceinline__ uint64_t bucket_end(const In& I) {
    const uint64_t b = I.first[1];
    return b < I.n ? b : I.n;
}

struct Rec {
    bool valid, head, last;
    uint32_t pay_off_lo, pay_off_hi, pay_len, seq, ack, conn, flags;
    uint32_t next, window, room, cap, snd_una, mss, cflags;   // the connection's state as given
    bool known;                                                // conn < nconns
};

__device__ __forceinline__ Rec load_rec(const In& I, uint64_t p, uint64_t end, bool with_state) {
    Rec r{};
    r.valid = p < end;
    if (!r.valid) return r;
    const uint2 a = I.seg[4 * p], b = I.seg[4 * p + 1], c = I.seg[4 * p + 2], d = I.seg[4 * p + 3];
    r.pay_off_lo = a.x;
    r.pay_off_hi = a.y;
    r.pay_len = b.x;
    r.seq = b.y;
    r.ack = c.x;
    r.conn = c.y;
    r.flags = (d.y >> 16) & 0xFFu;
    r.head = p == 0 || I.seg[4 * (p - 1) + 2].y != r.conn;
    r.last = p + 1 == end || I.seg[4 * (p + 1) + 2].y != r.conn;
    r.known = r.conn < I.nconns;   // a record of another bucket's conn never reads the state
    if (r.known) {
        const uint4 w1 = I.rcv[2 * uint64_t(r.conn) + 1];
        r.snd_una = w1.x;
        r.mss = w1.y & 0xFFFFu;
        r.cflags = (w1.y >> 16) & 0xFFu;
        if (with_state) {
            const uint4 w0 = I.rcv[2 * uint64_t(r.conn)];
            r.next = w0.x;
            r.window = w0.y;
            r.room = w0.z < kClamp ? w0.z : kClamp;
            r.cap = w0.w < kClamp ? w0.w : kClamp;
        }
    }
    return r;
}

// The record's element of the run scan.
__device__ __forceinline__ Elem elem_of(const Rec& r) {
    if (!r.valid) return Elem{0, kIdent};
    uint32_t meta = table_of(r.pay_len, r.mss);
    if (r.head) meta |= kHead | (threadIdx.x << kPosShift);
    return Elem{r.pay_len, meta};
}

// The run scan of the tile with what the run entering it brings: inclusive of
// the record.  meta keeps kHead and the head's thread for runs begun in the tile.
__device__ __forceinline__ Elem run_scan(const Rec& r, const Ws& W, Elem* part) {
    Elem total;
    Elem v = block_scan(elem_of(r), Elem{0, kIdent}, part, &total, SegSum{});
    if (!(v.meta & kHead)) v = SegSum{}(Elem{W.in_sum[blockIdx.x], W.in_meta[blockIdx.x]}, v);
    return v;
}

__device__ __forceinline__ uint32_t room_after(uint32_t room, uint64_t s) {
    return s < room ? room - static_cast<uint32_t>(s) : 0u;
}

// A record's term of the plain scan over the tile: the taken bytes (a tile holds
// less than 2^42), the taken records and the run heads (at most 1 024 each).
constexpr int kTakenShift = 42, kHeadsShift = 53;
__device__ __forceinline__ uint64_t packed(bool taken, bool head, uint32_t pay_len) {
    return (taken ? uint64_t(pay_len) | (uint64_t(1) << kTakenShift) : uint64_t(0)) |
           (head ? uint64_t(1) << kHeadsShift : uint64_t(0));
}
__device__ __forceinline__ uint64_t bytes_of(uint64_t x) { return x & ((uint64_t(1) << kTakenShift) - 1); }
__device__ __forceinline__ uint32_t taken_of(uint64_t x) { return static_cast<uint32_t>(x >> kTakenShift) & 0x7FFu; }
__device__ __forceinline__ uint32_t heads_of(uint64_t x) { return static_cast<uint32_t>(x >> kHeadsShift); }

// The first stop that holds for the record when the run's `s` bytes before it
// were all taken (sccsum.h's table, in its order); 0 when it is taken.
__device__ __forceinline__ uint32_t stop_of(const Rec& r, uint64_t s) {
    if (!r.known || !(r.cflags & SCCSUM_TCP_RCV_ELIGIBLE)) return SCCSUM_TCP_STOP_INELIGIBLE;
    const uint32_t room = room_after(r.room, s);
    const uint32_t window = r.head ? r.window : (room < r.cap ? room : r.cap);
    if (r.pay_len > 0 && window == 0) return SCCSUM_TCP_STOP_WINDOW;
    if (r.seq != r.next + static_cast<uint32_t>(s)) return SCCSUM_TCP_STOP_SEQ;
    if ((r.flags & 0x37u) != 0x10u) return SCCSUM_TCP_STOP_FLAGS;
    if (r.ack != r.snd_una) return SCCSUM_TCP_STOP_ACK;
    if (r.pay_len == 0) return SCCSUM_TCP_STOP_EMPTY;
    return 0;
}

// ---------------------------------------------------------------- the kernels

__global__ __launch_bounds__(kBlock) void sum_tile(In I, Ws W) {
    __shared__ Elem part[kWaves];
    const uint64_t end = bucket_end(I);
    const uint64_t p = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    if (uint64_t(blockIdx.x) * kTile >= end) return;  // the whole block
    const Rec r = load_rec(I, p, end, false);
    Elem total;
    (void)block_scan(elem_of(r), Elem{0, kIdent}, part, &total, SegSum{});
    const int heads = __syncthreads_count(r.valid && r.head);
    if (threadIdx.x == 0) {
        W.agg_sum[blockIdx.x] = total.sum;
        W.agg_meta[blockIdx.x] = total.meta & (0xFFFFu | kHead);
        W.heads[blockIdx.x] = static_cast<uint32_t>(heads);
    }
}

// ONE block: entry t of the carries is what the tiles before t leave.
__global__ __launch_bounds__(kBlock) void sum_carry(In I, Ws W) {
    __shared__ Elem part[kWaves];
    __shared__ uint32_t hpart[kWaves];
    const uint32_t ntiles = I.n ? static_cast<uint32_t>(tiles_of(bucket_end(I), kTile)) : 0u;
    Elem carry{0, kIdent};
    uint32_t hcarry = 0;
    if (threadIdx.x == 0) {
        W.in_sum[0] = 0;
        W.in_meta[0] = kIdent;
        W.heads_before[0] = 0;
    }
    for (uint32_t base = 0; base < ntiles; base += kBlock) {
        const uint32_t t = base + threadIdx.x;
        const bool live = t < ntiles;
        const Elem e = live ? Elem{W.agg_sum[t], W.agg_meta[t]} : Elem{0, kIdent};
        Elem total;
        Elem v = block_scan(e, Elem{0, kIdent}, part, &total, SegSum{});
        v = SegSum{}(carry, v);
        uint32_t htotal;
        const uint32_t h = hcarry + block_inclusive_scan<kWaves>(live ? W.heads[t] : 0u, hpart, &htotal);
        if (live) {
            W.in_sum[t + 1] = v.sum;
            W.in_meta[t + 1] = v.meta & 0xFFFFu;
            W.heads_before[t + 1] = h;
        }
        carry = SegSum{}(carry, total);
        hcarry += htotal;
    }
}

__global__ __launch_bounds__(kBlock) void stop_tile(In I, Ws W) {
    __shared__ Elem part[kWaves];
    __shared__ uint32_t cpart[kWaves];
    __shared__ uint64_t bpart[kWaves];
    const uint64_t end = bucket_end(I);
    const uint64_t p = uint64_t(blockIdx.x) * kTile + threadIdx.x;
    if (uint64_t(blockIdx.x) * kTile >= end) return;  // the whole block
    const Rec r = load_rec(I, p, end, true);
    const Elem v = run_scan(r, W, part);
    const bool bad = r.valid && stop_of(r, v.sum - r.pay_len) != 0;
    uint32_t ctotal;
    const uint32_t c = block_scan((r.valid && r.head ? 1u << 31 : 0u) | (bad ? 1u : 0u), 0u, cpart, &ctotal, SegCount{});
    const bool in_head = !(c >> 31);                         // the run came in from an earlier tile
    const bool taken = r.valid && (c & 0x7FFFFFFFu) == 0;    // ... unless that run came in stopped
    // one scan of the taken bytes, records and the heads; the tile's first head splits the totals
    __shared__ uint64_t before_first;
    const uint64_t x = packed(taken, r.valid && r.head, r.pay_len);
    uint64_t total;
    const uint64_t xi = block_inclusive_scan<kWaves>(x, bpart, &total);
    if (r.valid && r.head && heads_of(xi) == 1) before_first = xi - x;
    const int head_bad = __syncthreads_or(bad && in_head);
    if (threadIdx.x == 0) {
        const uint64_t h = heads_of(total) ? before_first : total;
        W.hbytes[blockIdx.x] = bytes_of(h);
        W.rbytes[blockIdx.x] = bytes_of(total) - bytes_of(h);
        W.hcnt[blockIdx.x] = taken_of(h);
        W.rcnt[blockIdx.x] = taken_of(total) - taken_of(h);
        W.tflags[blockIdx.x] = (head_bad ? 1u : 0u) | ((ctotal >> 31) ? 2u : 0u) | ((ctotal & 0x7FFFFFFFu) ? 4u : 0u);
    }
}

struct Out {
    uint2* run;              // sccsum_tcp_rcv_run as four 8-byte words
    uint2* desc;             // sccsum_gather_desc as two
    uint64_t* total;
    const uint32_t* run_first;
    const uint64_t* rx_total;
    uint64_t bytes;          // d_bytes as an address
    uint64_t max_bytes;
    uint64_t max_runs;       // min(n, nconns): what d_run holds besides R
};

// ONE block.  A tile's flags as a segmented OR: bit 1 a head, bit 0 stopped since.
struct SegOr {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const {
        return (b & 2u) ? b : (a & 2u) | ((a | b) & 1u);
    }
};

__global__ __launch_bounds__(kBlock) void stop_carry(In I, Ws W, Out O) {
    __shared__ uint32_t opart[kWaves];
    __shared__ uint64_t bpart[kWaves];
    __shared__ uint32_t shifted[kBlock];
    __shared__ uint32_t found;
    const uint32_t ntiles = I.n ? static_cast<uint32_t>(tiles_of(bucket_end(I), kTile)) : 0u;
    if (threadIdx.x == 0) found = 0;
    uint32_t ocarry = 0;
    uint64_t bcarry = 0, ccarry = 0;
    for (uint32_t base = 0; base < ntiles; base += kBlock) {
        const uint32_t t = base + threadIdx.x;
        const bool live = t < ntiles;
        const uint32_t tf = live ? W.tflags[t] : 0u;
        // the run leaving tile t has stopped: since the tile's last head, or before its first and on
        const uint32_t leave = (tf & 2u) | ((tf & 2u) ? (tf >> 2) & 1u : (tf | (tf >> 2)) & 1u);
        uint32_t ototal;
        uint32_t o = block_scan(leave, 0u, opart, &ototal, SegOr{});
        o = SegOr{}(ocarry, o);
        shifted[threadIdx.x] = o;
        __syncthreads();
        const uint32_t before = threadIdx.x ? shifted[threadIdx.x - 1] : ocarry;
        const bool stopped = (before & 1u) != 0;
        const uint64_t bytes = live ? W.rbytes[t] + (stopped ? uint64_t(0) : W.hbytes[t]) : uint64_t(0);
        const uint64_t cnt = live ? uint64_t(W.rcnt[t]) + (stopped ? 0u : W.hcnt[t]) : uint64_t(0);
        uint64_t btotal, ctotal;
        const uint64_t bi = bcarry + block_inclusive_scan<kWaves>(bytes, bpart, &btotal);
        const uint64_t ci = ccarry + block_inclusive_scan<kWaves>(cnt, bpart, &ctotal);
        if (live) {
            W.stopped_in[t] = stopped ? 1u : 0u;
            W.bytes_in[t] = bi - bytes;
            W.cnt_in[t] = ci - cnt;
            // the one tile where the packed text passes max_bytes: the run of the record that
            // passes it is the first that does not fit
            if (bi - bytes <= O.max_bytes && bi > O.max_bytes) {
                found = 1;
                const uint32_t hb = W.heads_before[t];  // 1..R with sccsum_tcp_rx's own outputs
                if (!stopped && hb != 0 && hb <= O.max_runs && bi - bytes + W.hbytes[t] > O.max_bytes) {
                    W.cut[0] = kCutAt;     // it came in from an earlier tile: its head is the last one before
                    W.cut[1] = O.run_first[hb - 1u];
                } else {
                    W.cut[0] = kCutInTile; // it begins in this tile, which finds its head
                    W.cut[1] = t * kTile;
                }
                W.cut[2] = t;
            }
        }
        ocarry = SegOr{}(ocarry, ototal);
        bcarry += btotal;
        ccarry += ctotal;
        __syncthreads();  // shifted is read no more
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (!found) {
            W.cut[0] = kCutNone;
            W.cut[1] = 0xFFFFFFFFu;
            W.cut[2] = 0xFFFFFFFFu;
            O.total[0] = ccarry;
            O.total[1] = bcarry;
        }  // else the record at the cut writes what is emitted before it
        O.total[2] = bcarry;
        O.total[3] = 0;
    }
}

__device__ __forceinline__ void store_run(uint2* run, uint64_t r, uint32_t taken, uint32_t bytes, uint32_t next,
                                          uint32_t window, uint32_t room, uint32_t desc_first, uint32_t dst_off,
                                          uint32_t flags, uint32_t stop) {
    run[4 * r] = make_uint2(taken, bytes);
    run[4 * r + 1] = make_uint2(next, window);
    run[4 * r + 2] = make_uint2(room, desc_first);
    run[4 * r + 3] = make_uint2(dst_off, flags | (stop << 8));
}

__global__ __launch_bounds__(kBlock) void place(In I, Ws W, Out O) {
    __shared__ Elem part[kWaves];
    __shared__ uint32_t cpart[kWaves];
    __shared__ uint64_t bpart[kWaves];
    __shared__ uint16_t tables[kBlock];
    __shared__ uint64_t cut_at;
    const uint64_t end = bucket_end(I);
    const uint64_t tile0 = uint64_t(blockIdx.x) * kTile;
    const uint64_t p = tile0 + threadIdx.x;
    if (tile0 >= end) return;  // the whole block
    const Rec r = load_rec(I, p, end, true);
    const Elem v = run_scan(r, W, part);
    const uint64_t s = v.sum - r.pay_len;   // the run's bytes before the record
    const uint32_t stop = r.valid ? stop_of(r, s) : 0u;
    const bool bad = stop != 0;
    uint32_t ctotal;
    uint32_t c = block_scan((r.valid && r.head ? 1u << 31 : 0u) | (bad ? 1u : 0u), 0u, cpart, &ctotal, SegCount{});
    if (!(c >> 31)) c += W.stopped_in[blockIdx.x];
    const uint32_t stops = c & 0x7FFFFFFFu;  // of the run, up to and with the record
    const bool taken = r.valid && stops == 0;
    // before the record, of the whole bucket: the taken bytes and records; the run heads up to it
    uint64_t xtotal;
    const uint64_t xi = block_inclusive_scan<kWaves>(packed(taken, r.valid && r.head, r.pay_len), bpart, &xtotal);
    const uint64_t bi = W.bytes_in[blockIdx.x] + bytes_of(xi);
    const uint64_t before_bytes = bi - (taken ? r.pay_len : 0u);
    const uint64_t before_cnt = W.cnt_in[blockIdx.x] + taken_of(xi) - (taken ? 1u : 0u);
    const uint64_t run_index = uint64_t(W.heads_before[blockIdx.x]) + heads_of(xi) - 1u;

    // the cut: the first position of the first run that does not fit
    const uint32_t kind = W.cut[0];
    if (threadIdx.x == 0) {
        cut_at = kind == kCutNone || (kind == kCutInTile && blockIdx.x < W.cut[2]) ? ~uint64_t(0) : uint64_t(W.cut[1]);
    }
    tables[threadIdx.x] = static_cast<uint16_t>(v.meta);
    __syncthreads();
    if (kind == kCutInTile && blockIdx.x == W.cut[2] && taken && before_bytes <= O.max_bytes && bi > O.max_bytes) {
        cut_at = tile0 + (v.meta >> kPosShift);   // one record passes max_bytes; its run began in this tile
    }
    __syncthreads();
    const uint64_t cut = cut_at;
    if (r.valid && p == cut) {
        O.total[0] = before_cnt;
        O.total[1] = before_bytes;
    }
    if (taken && p < cut) {
        const uint64_t src = O.bytes + ((uint64_t(r.pay_off_hi) << 32) | r.pay_off_lo);
        O.desc[2 * before_cnt] = make_uint2(static_cast<uint32_t>(src), static_cast<uint32_t>(src >> 32));
        O.desc[2 * before_cnt + 1] = make_uint2(static_cast<uint32_t>(before_bytes), r.pay_len);
    }
    // the run's record: written by its first record that stops, or by its last one
    if (!r.valid || !((bad && stops == 1) || (r.last && stops == 0))) return;
    if (run_index >= O.rx_total[0] || run_index >= O.max_runs) return;  // never with sccsum_tcp_rx's own outputs
    const uint64_t start = O.run_first[run_index];
    const uint32_t state0 = r.known ? (r.cflags & (SCCSUM_TCP_RCV_NR_FULL | SCCSUM_TCP_RCV_ACK_ARMED)) : 0u;
    if (start >= cut) {
        store_run(O.run, run_index, 0, 0, r.next, r.window, r.room, 0, 0, state0, SCCSUM_TCP_STOP_CAPACITY);
        return;
    }
    const uint64_t sum = bad ? s : v.sum;
    const uint32_t n_taken = static_cast<uint32_t>(p - start) + (bad ? 0u : 1u);
    uint32_t table = kIdent;
    if (!bad) {
        table = v.meta & 0xFFFFu;
    } else if (!r.head) {
        table = threadIdx.x ? tables[threadIdx.x - 1] : W.in_meta[blockIdx.x] & 0xFFFFu;
    }
    const uint32_t s0 = ((state0 & SCCSUM_TCP_RCV_NR_FULL) ? 1u : 0u) | ((state0 & SCCSUM_TCP_RCV_ACK_ARMED) ? 2u : 0u);
    const uint32_t e = (table >> (4 * s0)) & 15u;
    const uint32_t flags = ((e & 1u) ? SCCSUM_TCP_RCV_NR_FULL : 0u) | ((e & 2u) ? SCCSUM_TCP_RCV_ACK_ARMED : 0u) |
                           ((e & 4u) ? SCCSUM_TCP_RCV_ACK_REARMED : 0u) | ((e & 8u) ? SCCSUM_TCP_RCV_ACK_NOW : 0u);
    const uint32_t room = room_after(r.room, sum);
    const uint32_t window = n_taken ? (room < r.cap ? room : r.cap) : r.window;
    store_run(O.run, run_index, n_taken, static_cast<uint32_t>(sum), r.next + static_cast<uint32_t>(sum), window, room,
              static_cast<uint32_t>(before_cnt - (bad ? n_taken : n_taken - 1u)),
              static_cast<uint32_t>(before_bytes - (bad ? sum : sum - r.pay_len)), flags, stop);
}

// The runs from the cut onward take nothing: the exclusive scans stand at the totals.
__global__ __launch_bounds__(kFlatBlock) void cut_runs(Out O) {
    const uint64_t r = uint64_t(blockIdx.x) * kFlatBlock + threadIdx.x;
    if (r >= O.rx_total[0] || r >= O.max_runs) return;
    if (((O.run[4 * r + 3].y >> 8) & 0xFFu) != SCCSUM_TCP_STOP_CAPACITY) return;
    O.run[4 * r + 2].y = static_cast<uint32_t>(O.total[0]);
    O.run[4 * r + 3].x = static_cast<uint32_t>(O.total[1]);
}

// ---------------------------------------------------------------- host side

// The workspace: 8-byte things first.
struct Layout {
    uint64_t agg_sum, in_sum, hbytes, rbytes, bytes_in, cnt_in;
    uint64_t agg_meta, heads, in_meta, heads_before, hcnt, rcnt, tflags, stopped_in, cut, bytes;
};

Layout layout_of(uint64_t n) {
    Layout L{};
    const uint64_t k = tiles_of(n, kTile) + 1;
    host_launch::Carver c;
    uint64_t* const wide[] = {&L.agg_sum, &L.in_sum, &L.hbytes, &L.rbytes, &L.bytes_in, &L.cnt_in};
    for (uint64_t* w : wide) *w = c.take(8 * k);
    uint64_t* const narrow[] = {&L.agg_meta, &L.heads, &L.in_meta, &L.heads_before, &L.hcnt, &L.rcnt, &L.tflags,
                                &L.stopped_in};
    for (uint64_t* w : narrow) *w = c.take(4 * k);
    L.cut = c.take(16);
    L.bytes = c.end();
    return L;
}

}  // namespace tcp_data

extern "C" {

uint64_t sccsum_tcp_rx_data_workspace(uint64_t n, uint32_t nconns) {
    (void)nconns;  // everything is per tile
    return tcp_data::layout_of(n).bytes;
}

int sccsum_tcp_rx_data(const void* d_bytes, const sccsum_tcp_seg* d_seg, const uint32_t* d_first,
                       const uint32_t* d_run_conn, const uint32_t* d_run_first, const uint64_t* d_rx_total, uint64_t n,
                       const sccsum_tcp_rcv* d_rcv, uint32_t nconns, uint64_t max_bytes, sccsum_tcp_rcv_run* d_run,
                       sccsum_gather_desc* d_desc, uint64_t* d_total, void* d_workspace, void* stream) {
    using namespace tcp_data;
    if (n > 0xFFFFFFFFull || nconns > SCCSUM_TCP_MAX_CONNS || max_bytes > 0xFFFFFFFFull) return SCCSUM_EINVAL;
    if (!d_total || !d_workspace || misaligned(d_total, 8) || misaligned(d_workspace, 16)) return SCCSUM_EINVAL;
    if (n != 0) {
        if (!d_seg || !d_first || !d_run_conn || !d_run_first || !d_rx_total || !d_run || !d_desc) return SCCSUM_EINVAL;
        if (nconns != 0 && !d_rcv) return SCCSUM_EINVAL;
        if (misaligned(d_seg, 8) || misaligned(d_first, 4) || misaligned(d_run_conn, 4) || misaligned(d_run_first, 4) ||
            misaligned(d_rx_total, 8) || misaligned(d_rcv, 16) || misaligned(d_run, 8) || misaligned(d_desc, 8)) {
            return SCCSUM_EINVAL;
        }
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, -1);
    if (rc != SCCSUM_OK) return rc;

    const Layout L = layout_of(n);
    const Workspace ws(d_workspace);
    const Ws W{ws.u64(L.agg_sum), ws.u32(L.agg_meta), ws.u32(L.heads), ws.u64(L.in_sum), ws.u32(L.in_meta),
               ws.u32(L.heads_before), ws.u64(L.hbytes), ws.u64(L.rbytes), ws.u32(L.hcnt), ws.u32(L.rcnt),
               ws.u32(L.tflags), ws.u64(L.bytes_in), ws.u64(L.cnt_in), ws.u32(L.stopped_in), ws.u32(L.cut)};
    const In I{reinterpret_cast<const uint2*>(d_seg), d_first, reinterpret_cast<const uint4*>(d_rcv), n, nconns};
    const uint64_t runs = n < nconns ? n : nconns;
    const Out O{reinterpret_cast<uint2*>(d_run), reinterpret_cast<uint2*>(d_desc), d_total, d_run_first, d_rx_total,
                reinterpret_cast<uint64_t>(d_bytes), max_bytes, runs};
    const dim3 tiles(static_cast<unsigned>(tiles_of(n, kTile))), block(kBlock);
    Chain c{st};
    if (n != 0) {
        c.launch(sum_tile, tiles, block, 0, I, W);
        c.launch(sum_carry, dim3(1), block, 0, I, W);
        c.launch(stop_tile, tiles, block, 0, I, W);
    }
    c.launch(stop_carry, dim3(1), block, 0, I, W, O);
    if (n == 0) return c.rc();
    c.launch(place, tiles, block, 0, I, W, O);
    if (runs == 0) return c.rc();
    const uint64_t blocks = (runs + kFlatBlock - 1) / kFlatBlock;
    c.launch(cut_runs, dim3(static_cast<unsigned>(blocks)), dim3(kFlatBlock), 0, O);
    return c.rc();
}

}  // extern "C"
