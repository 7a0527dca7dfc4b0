// tcp_ack.hip — the TCP ACK fast path on the GPU: the leading stretch of
// advancing pure ACKs of every connection's run of sccsum_tcp_rx's bucket 0
// (sccsum.h, "TCP ACK fast path").
//
// What it restates from the reference (paths relative to the reference tree):
//   tcb::segment_acceptable, seg_len == 0   include/seastar/net/tcp.hh:1058-1064
//   tcb::input_handle_other_state           tcp.hh:1215-1575, of which only the
//                                           advancing-ACK branch (tcp.hh:1336-1400,
//                                           dupacks < 3) and the closing output()
//                                           (tcp.hh:1570-1574) do anything here
//   tcb::data_segment_acked                 tcp.hh:1026-1055
//   tcb::update_rto, update_cwnd            tcp.hh:2016-2039, 2042-2052
//   update_window                           tcp.hh:1316-1329
//   tcb::can_send                           tcp.hh:515-549
//
// Whether a segment leaves the straight path is a function of the segment, its
// predecessor in the run and the connection's record as given: while every
// earlier ACK was taken, SND.UNA is the predecessor's ack, SND.WL1 / WL2 are its
// seq / ack and nothing else the tests read has moved.  So every record's stop
// is evaluated in parallel, and the run's walk ends at the first one set.
//
// Plain dependent launches on the caller's stream, no block waiting on another
// one and no atomic:
//   scan_array   twice over the queue entries (array_scan.h): the 64-bit
//                exclusive scan G of the lengths (a queue's length and an entry's
//                end inside it are differences of it) and the count Z of
//                entries of no bytes
//   eval         per record: its stop, or ack - una, the scaled window and the
//                can_send() bit behind it, as one 8-byte pair
//   walk         one lane per run: the pairs up to the first stop merged with
//                the entries' ends, through data_segment_acked; the run record;
//                the block's sums
//   totals       ONE block: d_total
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "array_scan.h"
#include "host_launch.h"
#include "sccsum.h"
#include "wave_scan.h"
#include "wire.h"

namespace tcp_ack {

using array_scan::scan_array;
using host_launch::Chain;
using host_launch::misaligned;
using host_launch::stream_ok;
using host_launch::Workspace;
using wave_scan::block_inclusive_scan;
using wire::tiles_of;

constexpr int kWave = 64;
constexpr int kBlock = 256;                  // threads of both kernels: one record, one run each
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kBad = 1u << 31;          // Pair::y: the record stops the run, the low byte says why
constexpr uint32_t kCanSend = 1u << 30;      // ... else can_send() > 0 behind it; the window is below 2^30
constexpr uint64_t kMaxEntries = uint64_t(1) << 31;

static_assert(sizeof(sccsum_tcp_ack) == 64 && sizeof(sccsum_tcp_ack_run) == 64 && sizeof(sccsum_tcp_seg) == 32, "layout");
static_assert(offsetof(sccsum_tcp_ack, wl2) == 16 && offsetof(sccsum_tcp_ack, rcv_next) == 32 &&
                  offsetof(sccsum_tcp_ack, srtt) == 40 && offsetof(sccsum_tcp_ack, rttvar) == 48 &&
                  offsetof(sccsum_tcp_ack, mss) == 56 && offsetof(sccsum_tcp_ack, flags) == 59 &&
                  offsetof(sccsum_tcp_ack_run, trim) == 16 && offsetof(sccsum_tcp_ack_run, srtt) == 32 &&
                  offsetof(sccsum_tcp_ack_run, rto) == 48 && offsetof(sccsum_tcp_ack_run, flags) == 52 &&
                  offsetof(sccsum_tcp_ack_run, stop) == 53,
              "the kernels read and write the records as 16-byte words");

struct LoadZero {
    const uint32_t* len;
    __device__ __forceinline__ uint32_t operator()(uint64_t j) const { return len[j] == 0 ? 1u : 0u; }
};

struct In {
    const uint2* seg;        // sccsum_tcp_seg as four 8-byte words: d_seg is 8-byte aligned
    const uint32_t* first;   // d_first of sccsum_tcp_rx: bucket 0 is [0, first[1])
    const uint4* ack;        // sccsum_tcp_ack as four 16-byte words
    const uint32_t* q_first;
    const uint64_t* G;       // workspace: the exclusive scan of d_q_len, nq + 1 entries
    const uint32_t* Z;       // ... and of its entries of no bytes
    uint64_t n;
    uint32_t nconns;
    uint32_t nq;
};

__device__ __forceinline__ uint64_t bucket_end(const In& I) {
    const uint64_t b = I.first[1];
    return b < I.n ? b : I.n;
}

// The connection's record as given and its queue, inside [0, nq] whatever q_first says.
struct Conn {
    uint32_t una, next, window, wl1, wl2, cwnd, ssthresh, unsent_len, rcv_next, rto;
    int64_t srtt, rttvar;
    uint32_t mss, window_scale, flags;
    uint32_t qa, qb;
    uint32_t stop;           // 0, _STOP_INELIGIBLE or _STOP_QUEUE: the whole run's
};

__device__ __forceinline__ Conn load_conn(const In& I, uint32_t c) {
    Conn r{};
    if (c >= I.nconns) {
        r.stop = SCCSUM_TCP_STOP_INELIGIBLE;
        return r;
    }
    const uint4 w0 = I.ack[4 * uint64_t(c)], w1 = I.ack[4 * uint64_t(c) + 1], w2 = I.ack[4 * uint64_t(c) + 2],
                w3 = I.ack[4 * uint64_t(c) + 3];
    r.una = w0.x;
    r.next = w0.y;
    r.window = w0.z;
    r.wl1 = w0.w;
    r.wl2 = w1.x;
    r.cwnd = w1.y;
    r.ssthresh = w1.z;
    r.unsent_len = w1.w;
    r.rcv_next = w2.x;
    r.rto = w2.y;
    r.srtt = static_cast<int64_t>((uint64_t(w2.w) << 32) | w2.z);
    r.rttvar = static_cast<int64_t>((uint64_t(w3.y) << 32) | w3.x);
    r.mss = w3.z & 0xFFFFu;
    r.window_scale = (w3.z >> 16) & 0xFFu;
    r.flags = w3.z >> 24;
    if (!(r.flags & SCCSUM_TCP_ACK_ELIGIBLE) || r.window == 0 || r.cwnd == 0 || r.cwnd >= (1u << 31) ||
        r.window_scale > 14 || static_cast<int32_t>(r.next - r.una) < 0) {
        r.stop = SCCSUM_TCP_STOP_INELIGIBLE;
        return r;
    }
    const uint32_t a = I.q_first[c], b = I.q_first[c + 1];
    r.qa = a < I.nq ? a : I.nq;
    r.qb = b < r.qa ? r.qa : b < I.nq ? b : I.nq;
    if (I.G[r.qb] - I.G[r.qa] != uint64_t(r.next - r.una) || I.Z[r.qb] != I.Z[r.qa]) r.stop = SCCSUM_TCP_STOP_QUEUE;
    return r;
}

// tcp_seq's order (tcp.hh:220-226).
__device__ __forceinline__ bool seq_lt(uint32_t a, uint32_t b) { return static_cast<int32_t>(a - b) < 0; }
__device__ __forceinline__ bool seq_le(uint32_t a, uint32_t b) { return static_cast<int32_t>(a - b) <= 0; }

// ---------------------------------------------------------------- the kernels

// Per record of bucket 0: pair[p] = {ack - una as given, kBad | stop} or {.., window | kCanSend}.
__global__ __launch_bounds__(kBlock) void eval(In I, uint2* __restrict__ pair) {
    const uint64_t end = bucket_end(I);
    const uint64_t p = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= end) return;
    const uint2 b = I.seg[4 * p + 1], c = I.seg[4 * p + 2], d = I.seg[4 * p + 3];
    const uint32_t pay_len = b.x, seq = b.y, ack = c.x, conn = c.y;
    const uint32_t window16 = d.x & 0xFFFFu, flags = (d.y >> 16) & 0xFFu;
    const uint2 before = p ? I.seg[4 * (p - 1) + 2] : make_uint2(0, 0);
    const bool head = p == 0 || before.y != conn;
    const Conn k = load_conn(I, conn);
    const uint32_t prev = head ? k.una : before.x;
    const uint32_t window = window16 << k.window_scale;   // at most 0xFFFF << 14
    const auto stop_of = [&]() -> uint32_t {   // sccsum.h's table, in its order
        if (k.stop) return k.stop;
        if (seq != k.rcv_next) return SCCSUM_TCP_STOP_SEQ;
        if ((flags & 0x37u) != 0x10u) return SCCSUM_TCP_STOP_FLAGS;
        if (pay_len != 0) return SCCSUM_TCP_STOP_DATA;
        if (!(seq_lt(prev, ack) && seq_le(ack, k.next))) return SCCSUM_TCP_STOP_ACK;
        if (head && !(seq_lt(k.wl1, seq) || (k.wl1 == seq && seq_le(k.wl2, ack)))) return SCCSUM_TCP_STOP_WL;
        if (window == 0) return SCCSUM_TCP_STOP_WINDOW;
        return 0u;
    };
    const uint32_t stop = stop_of();
    const bool can_send = k.unsent_len > 0 && k.next - ack < window;
    pair[p] = make_uint2(ack - k.una, stop ? kBad | stop : window | (can_send ? kCanSend : 0u));
}

struct Out {
    uint4* run;              // sccsum_tcp_ack_run as four 16-byte words
    uint64_t* total;
    const uint32_t* run_conn;
    const uint32_t* run_first;
    const uint64_t* rx_total;
    const uint32_t* q_len;
    const uint32_t* q_meta;
    const int64_t* q_tx;
    int64_t now_ns;
    uint64_t max_runs;       // min(n, nconns): what d_run holds
    uint64_t* t_taken;       // workspace, per block of walk
    uint64_t* t_popped;
    uint64_t* t_acked;
};

// One lane per run.  The walk is the reference's loop: the taken ACKs in
// order, each popping the entries that end at or before it.
__global__ __launch_bounds__(kBlock) void walk(In I, const uint2* __restrict__ pair, Out O) {
    __shared__ uint64_t part[kWaves];
    const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    const uint64_t runs = O.rx_total[0] < O.max_runs ? O.rx_total[0] : O.max_runs;
    uint64_t taken = 0, popped = 0, acked = 0;
    if (r < runs) {
        const uint64_t end = bucket_end(I);
        const uint64_t f0 = O.run_first[r], f1 = O.run_first[r + 1];
        const uint64_t lo = f0 < end ? f0 : end;
        const uint64_t hi = f1 < lo ? lo : f1 < end ? f1 : end;
        const Conn k = load_conn(I, O.run_conn[r]);
        uint32_t off = 0;                    // una - una as given
        uint32_t trim = 0, freed = 0, window = k.window, cwnd = k.cwnd, rto = k.rto, poll = 0;
        int64_t srtt = k.srtt, rttvar = k.rttvar;
        bool first_sample = (k.flags & SCCSUM_TCP_ACK_FIRST_SAMPLE) != 0;
        uint64_t j = k.qa;
        const uint64_t base = I.G[k.qa];
        uint32_t stop = SCCSUM_TCP_STOP_END;
        const auto update_cwnd = [&](uint32_t bytes) {
            if (cwnd < k.ssthresh) {
                cwnd += bytes < k.mss ? bytes : k.mss;
            } else {
                const uint32_t q = k.mss * k.mss / cwnd;
                cwnd += q > 1u ? q : 1u;
            }
        };
        for (uint64_t i = lo; i < hi; ++i) {
            const uint2 a = pair[i];
            if (a.y & kBad) {
                stop = a.y & 0xFFu;
                break;
            }
            // full ACK of entries (tcp.hh:1029-1042): una + len <= ack is "the entry ends at or before ack"
            while (j < k.qb && I.G[j + 1] - base <= a.x) {
                const uint32_t end_off = static_cast<uint32_t>(I.G[j + 1] - base);
                const uint32_t len = end_off - off;   // what is left of it: p.len() after the trims
                const uint32_t meta = O.q_meta[j];
                off = end_off;
                if (!(meta & 0x10000u)) {
                    const int64_t R = (O.now_ns - O.q_tx[j]) / 1000000;
                    if (first_sample) {
                        first_sample = false;
                        rttvar = R / 2;
                        srtt = R;
                    } else {
                        const int64_t delta = srtt > R ? srtt - R : R - srtt;
                        rttvar = rttvar * 3 / 4 + delta / 4;
                        srtt = srtt * 7 / 8 + R / 8;
                    }
                    const int64_t v = 4 * rttvar > 1 ? 4 * rttvar : 1;
                    const int64_t t = srtt + v;
                    rto = static_cast<uint32_t>(t < 1000 ? 1000 : t > 60000 ? 60000 : t);
                }
                update_cwnd(len);
                freed += meta & 0xFFFFu;
                trim = 0;
                ++popped;
                ++j;
            }
            // partial ACK of the front entry (tcp.hh:1044-1053)
            if (off < a.x) {
                const uint32_t partial = a.x - off;
                trim += partial;
                off = a.x;
                update_cwnd(partial);
            }
            window = a.y & (kCanSend - 1u);
            poll |= a.y & kCanSend;
            ++taken;
        }
        acked = off;
        uint32_t flags = first_sample ? SCCSUM_TCP_ACK_FIRST_SAMPLE : 0u;
        if (taken) {
            flags |= j == k.qb ? SCCSUM_TCP_ACK_ALL_ACKED : SCCSUM_TCP_ACK_RTX_REARM;
            if (poll && !(k.flags & SCCSUM_TCP_ACK_CLOSE_WAIT)) flags |= SCCSUM_TCP_ACK_POLL;
        }
        O.run[4 * r] = make_uint4(static_cast<uint32_t>(taken), k.una + off, off, static_cast<uint32_t>(popped));
        O.run[4 * r + 1] = make_uint4(trim, freed, window, cwnd);
        O.run[4 * r + 2] = make_uint4(static_cast<uint32_t>(srtt), static_cast<uint32_t>(uint64_t(srtt) >> 32),
                                      static_cast<uint32_t>(rttvar), static_cast<uint32_t>(uint64_t(rttvar) >> 32));
        O.run[4 * r + 3] = make_uint4(rto, flags | (stop << 8), 0, 0);
    }
    uint64_t tt, tp, ta;
    (void)block_inclusive_scan<kWaves>(taken, part, &tt);
    (void)block_inclusive_scan<kWaves>(popped, part, &tp);
    (void)block_inclusive_scan<kWaves>(acked, part, &ta);
    if (threadIdx.x == 0) {
        O.t_taken[blockIdx.x] = tt;
        O.t_popped[blockIdx.x] = tp;
        O.t_acked[blockIdx.x] = ta;
    }
}

// ONE block: the blocks' sums of walk.
__global__ __launch_bounds__(kBlock) void totals(Out O, uint64_t nblocks) {
    __shared__ uint64_t part[kWaves];
    uint64_t taken = 0, popped = 0, acked = 0;
    for (uint64_t base = 0; base < nblocks; base += kBlock) {
        const uint64_t t = base + threadIdx.x;
        const bool live = t < nblocks;
        uint64_t tt, tp, ta;
        (void)block_inclusive_scan<kWaves>(live ? O.t_taken[t] : uint64_t(0), part, &tt);
        (void)block_inclusive_scan<kWaves>(live ? O.t_popped[t] : uint64_t(0), part, &tp);
        (void)block_inclusive_scan<kWaves>(live ? O.t_acked[t] : uint64_t(0), part, &ta);
        taken += tt;
        popped += tp;
        acked += ta;
    }
    if (threadIdx.x == 0) {
        const uint64_t runs = nblocks == 0 ? 0 : O.rx_total[0] < O.max_runs ? O.rx_total[0] : O.max_runs;
        O.total[0] = runs;
        O.total[1] = taken;
        O.total[2] = popped;
        O.total[3] = acked;
    }
}

// ---------------------------------------------------------------- host side

// The workspace: 8-byte things first.
struct Layout {
    uint64_t G, gt, pair, t_taken, t_popped, t_acked, Z, zt, bytes;
};

Layout layout_of(uint64_t n, uint64_t nconns, uint64_t nq) {
    Layout L{};
    const uint64_t qtiles = tiles_of(nq, array_scan::kTile) + 1;
    const uint64_t rblocks = tiles_of(n < nconns ? n : nconns, kBlock) + 1;
    host_launch::Carver c;
    L.G = c.take(8 * (nq + 1));
    L.gt = c.take(8 * qtiles);
    L.pair = c.take(8 * n);
    L.t_taken = c.take(8 * rblocks);
    L.t_popped = c.take(8 * rblocks);
    L.t_acked = c.take(8 * rblocks);
    L.Z = c.take(4 * (nq + 1));
    L.zt = c.take(4 * qtiles);
    L.bytes = c.end();
    return L;
}

}  // namespace tcp_ack

extern "C" {

uint64_t sccsum_tcp_rx_acks_workspace(uint64_t n, uint32_t nconns, uint64_t nq) {
    return tcp_ack::layout_of(n, nconns, nq).bytes;
}

int sccsum_tcp_rx_acks(const sccsum_tcp_seg* d_seg, const uint32_t* d_first, const uint32_t* d_run_conn,
                       const uint32_t* d_run_first, const uint64_t* d_rx_total, uint64_t n, const sccsum_tcp_ack* d_ack,
                       uint32_t nconns, const uint32_t* d_q_first, const uint32_t* d_q_len, const uint32_t* d_q_meta,
                       const int64_t* d_q_tx, uint64_t nq, int64_t now_ns, sccsum_tcp_ack_run* d_run, uint64_t* d_total,
                       void* d_workspace, void* stream) {
    using namespace tcp_ack;
    if (n > 0xFFFFFFFFull || nconns > SCCSUM_TCP_MAX_CONNS || nq > kMaxEntries) return SCCSUM_EINVAL;
    if (!d_total || !d_workspace || misaligned(d_total, 8) || misaligned(d_workspace, 16)) return SCCSUM_EINVAL;
    if (nconns != 0 && !d_q_first) return SCCSUM_EINVAL;
    if (n != 0) {
        if (!d_seg || !d_first || !d_run_conn || !d_run_first || !d_rx_total || !d_run) return SCCSUM_EINVAL;
        if (nconns != 0 && !d_ack) return SCCSUM_EINVAL;
        if (nq != 0 && (!d_q_len || !d_q_meta || !d_q_tx)) return SCCSUM_EINVAL;
        if (misaligned(d_seg, 8) || misaligned(d_first, 4) || misaligned(d_run_conn, 4) || misaligned(d_run_first, 4) ||
            misaligned(d_rx_total, 8) || misaligned(d_ack, 16) || misaligned(d_run, 16) || misaligned(d_q_first, 4) ||
            misaligned(d_q_len, 4) || misaligned(d_q_meta, 4) || misaligned(d_q_tx, 8)) {
            return SCCSUM_EINVAL;
        }
    }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = stream_ok(st, -1);
    if (rc != SCCSUM_OK) return rc;

    const Layout L = layout_of(n, nconns, nq);
    const Workspace ws(d_workspace);
    const uint64_t max_runs = n < nconns ? n : nconns;
    const uint64_t rblocks = tiles_of(max_runs, kBlock);
    const uint32_t entries = static_cast<uint32_t>(nconns ? nq : 0);   // without a connection no entry is read
    const In I{reinterpret_cast<const uint2*>(d_seg), d_first, reinterpret_cast<const uint4*>(d_ack), d_q_first,
               ws.u64(L.G), ws.u32(L.Z), n, nconns, entries};
    const Out O{reinterpret_cast<uint4*>(d_run), d_total, d_run_conn, d_run_first, d_rx_total, d_q_len, d_q_meta,
                d_q_tx, now_ns, max_runs, ws.u64(L.t_taken), ws.u64(L.t_popped), ws.u64(L.t_acked)};
    uint2* const pair = ws.at<uint2>(L.pair);
    Chain c{st};
    if (rblocks != 0) {
        c.e = scan_array<uint64_t>(st, array_scan::LoadLen{d_q_len}, entries, ws.u64(L.gt), ws.u64(L.G));
        if (c.ok()) c.e = scan_array<uint32_t>(st, LoadZero{d_q_len}, entries, ws.u32(L.zt), ws.u32(L.Z));
        c.launch(eval, dim3(static_cast<unsigned>(tiles_of(n, kBlock))), dim3(kBlock), 0, I, pair);
        c.launch(walk, dim3(static_cast<unsigned>(rblocks)), dim3(kBlock), 0, I, pair, O);
    }
    c.launch(totals, dim3(1), dim3(kBlock), 0, O, rblocks);
    return c.rc();
}

}  // extern "C"
