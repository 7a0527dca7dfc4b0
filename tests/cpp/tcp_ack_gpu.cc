// Native host program over the C++ class tcp_rx_acks
// (seastar/net/ip_checksum_batch.hh): run() forwards 18 arguments, many of one
// type, five of them taken from tcp_rx's outputs struct and five from its own
// queues struct, to a C call that the Python tests pin.  Here the wrapper and
// the C call run on the same inputs into two separately poisoned sets of
// outputs (64 guard bytes behind each array, the workspaces poisoned too), and
// every array must be byte-equal: a swapped or dropped argument, or a field
// mapped to the wrong parameter, shows.  The input is written as tcp_rx leaves
// it: 2 300 records of 97 connections in runs of mixed length, most of them
// advancing pure ACKs, some leaving the straight path (a gap, a FIN, text, a
// duplicate ACK, a closed window), one connection not eligible and one whose
// queue does not add up.
// Prints OK and exits 0; a mismatch prints the array's name and exits 1.
#include <hip/hip_runtime.h>
#include <seastar/net/ip_checksum_batch.hh>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace seastar::net;

namespace {

constexpr size_t kGuard = 64;
constexpr int kPoison = 0xA5;

void hip_ok(hipError_t e, const char* what, int line) {
    if (e != hipSuccess) {
        std::printf("HIP error %s (%s) at line %d\n", hipGetErrorString(e), what, line);
        std::exit(2);
    }
}
#define HIP_OK(x) hip_ok((x), #x, __LINE__)

// A device array of `bytes` bytes and kGuard more, all poisoned.
struct dev_array {
    uint8_t* p = nullptr;
    size_t bytes = 0;
    explicit dev_array(size_t n, int fill = kPoison) : bytes(n) {
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), n + kGuard));
        HIP_OK(hipMemset(p, fill, n + kGuard));
    }
    dev_array(const dev_array&) = delete;
    dev_array& operator=(const dev_array&) = delete;
    ~dev_array() { (void)hipFree(p); }
    template <typename T>
    T* as() const { return reinterpret_cast<T*>(p); }
    std::vector<uint8_t> host() const {
        std::vector<uint8_t> h(bytes + kGuard);
        HIP_OK(hipMemcpy(h.data(), p, h.size(), hipMemcpyDeviceToHost));
        return h;
    }
};

template <typename T>
void upload(const dev_array& d, const std::vector<T>& v) {
    if (!v.empty()) HIP_OK(hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}

int bad = 0;

// Both arrays byte for byte, guards included (both were poisoned alike), and the guards themselves.
void same(const char* name, const dev_array& a, const dev_array& b) {
    const std::vector<uint8_t> ha = a.host(), hb = b.host();
    if (ha != hb) {
        std::printf("MISMATCH %s\n", name);
        ++bad;
    }
    for (size_t k = 0; k < kGuard; ++k) {
        if (ha[a.bytes + k] != kPoison || hb[b.bytes + k] != kPoison) {
            std::printf("MISMATCH %s (guard bytes written)\n", name);
            ++bad;
            break;
        }
    }
}

struct out_set {
    dev_array run, total, ws;
    out_set(uint64_t runs, uint64_t ws_bytes) : run(sizeof(sccsum_tcp_ack_run) * runs), total(8 * 4), ws(ws_bytes, 0x5A) {}
    tcp_rx_acks::outputs out() const {
        tcp_rx_acks::outputs o;
        o.run = run.as<sccsum_tcp_ack_run>();
        o.total = total.as<uint64_t>();
        return o;
    }
};

}  // namespace

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        std::printf("no device\n");
        return 2;
    }
    HIP_OK(hipSetDevice(0));
    hipStream_t stream;
    HIP_OK(hipStreamCreate(&stream));
    std::mt19937 rng(89);

    constexpr uint32_t kConns = 97, kOthers = 11;
    constexpr int64_t kNow = 7000000000;
    const uint64_t n0 = 2300, n = n0 + kOthers;
    std::vector<sccsum_tcp_ack> ack(kConns);
    std::vector<sccsum_tcp_seg> seg(n);
    std::vector<uint32_t> run_conn(kConns + 1), run_first(kConns + 1), q_first(kConns + 1), q_len, q_meta;
    std::vector<int64_t> q_tx;
    uint64_t p = 0;
    for (uint32_t c = 0; c < kConns; ++c) {
        const uint64_t count = c + 1 == kConns ? n0 - p : (c == 7 ? 1500 : 1 + rng() % 8);
        sccsum_tcp_ack& s = ack[c];
        s = sccsum_tcp_ack{};
        s.una = c == 5 ? 0xFFFFFFFFu : static_cast<uint32_t>(rng());
        s.window = 65535;
        s.rcv_next = static_cast<uint32_t>(rng());
        s.wl1 = s.rcv_next;
        s.wl2 = s.una;
        s.mss = 1460;
        s.cwnd = c % 2 ? 2920 : 1460 * 1460;
        s.ssthresh = c % 2 ? 8000 : 2920;
        s.unsent_len = c % 3 ? 100000 : 0;
        s.rto = 1000;
        s.srtt = 40;
        s.rttvar = 10;
        s.window_scale = static_cast<uint8_t>(c % 8);
        s.flags = static_cast<uint8_t>((c == 13 ? 0 : SCCSUM_TCP_ACK_ELIGIBLE) | (c % 5 == 4 ? SCCSUM_TCP_ACK_CLOSE_WAIT : 0) |
                                       (c % 4 == 0 ? SCCSUM_TCP_ACK_FIRST_SAMPLE : 0));
        // the queue: entries of 1..1500 bytes, half as many more as the run has ACKs
        q_first[c] = static_cast<uint32_t>(q_len.size());
        uint32_t flight = 0;
        for (uint64_t j = 0; j < count + count / 2 + 1; ++j) {
            const uint32_t len = 1 + rng() % 1500;
            q_len.push_back(len);
            q_meta.push_back(len | (rng() % 4 == 0 ? 0x10000u : 0u));
            q_tx.push_back(kNow - static_cast<int64_t>(rng() % 300) * 1000000 - static_cast<int64_t>(rng() % 1000000));
            flight += len;
        }
        s.next = s.una + flight + (c == 21 ? 1 : 0);   // connection 21's queue does not add up
        run_conn[c] = c;
        run_first[c] = static_cast<uint32_t>(p);
        uint32_t at = 0;
        for (uint64_t k = 0; k < count; ++k, ++p) {
            sccsum_tcp_seg& g = seg[p];
            g = sccsum_tcp_seg{};
            at += 1 + rng() % (flight / static_cast<uint32_t>(count));
            g.seq = s.rcv_next;
            g.ack = s.una + at;
            g.conn = c;
            g.window = static_cast<uint16_t>(1 + rng() % 65535);
            g.flags = 0x10 | (k % 5 == 0 ? 0x08 : 0);
            g.hdr_len = 20;
            if (c % 9 == 3 && k == 4) g.seq += 100;              // a gap
            if (c % 9 == 4 && k == 2) g.flags |= 0x01;           // FIN
            if (c % 9 == 5 && k == 3) g.pay_len = 10;            // text
            if (c % 9 == 6 && k == 1) g.ack = seg[p - 1].ack;    // a duplicate ACK
            if (c % 9 == 8 && k == 2) g.window = 0;              // a closed window
        }
    }
    q_first[kConns] = static_cast<uint32_t>(q_len.size());
    run_first[kConns] = static_cast<uint32_t>(n0);
    for (uint64_t k = n0; k < n; ++k) {
        seg[k] = sccsum_tcp_seg{};
        seg[k].conn = UINT32_MAX;
        seg[k].flags = 0x10;
    }
    const uint64_t nq = q_len.size();
    const std::vector<uint32_t> first = {0, static_cast<uint32_t>(n0), static_cast<uint32_t>(n0 + 4),
                                         static_cast<uint32_t>(n), static_cast<uint32_t>(n)};
    const std::vector<uint64_t> rx_total = {kConns, kOthers - 4, 0, 0};
    dev_array d_seg(sizeof(sccsum_tcp_seg) * n), d_ack(sizeof(sccsum_tcp_ack) * kConns), d_first(4 * 5),
        d_run_conn(4 * (kConns + 1)), d_run_first(4 * (kConns + 1)), d_rx_total(8 * 4), d_q_first(4 * (kConns + 1)),
        d_q_len(4 * nq), d_q_meta(4 * nq), d_q_tx(8 * nq);
    upload(d_seg, seg);
    upload(d_ack, ack);
    upload(d_first, first);
    upload(d_run_conn, run_conn);
    upload(d_run_first, run_first);
    upload(d_rx_total, rx_total);
    upload(d_q_first, q_first);
    upload(d_q_len, q_len);
    upload(d_q_meta, q_meta);
    upload(d_q_tx, q_tx);

    tcp_rx::outputs rx;
    rx.seg = d_seg.as<sccsum_tcp_seg>();
    rx.first = d_first.as<uint32_t>();
    rx.run_conn = d_run_conn.as<uint32_t>();
    rx.run_first = d_run_first.as<uint32_t>();
    rx.total = d_rx_total.as<uint64_t>();
    tcp_rx_acks::queues q;
    q.first = d_q_first.as<uint32_t>();
    q.len = d_q_len.as<uint32_t>();
    q.meta = d_q_meta.as<uint32_t>();
    q.tx = d_q_tx.as<int64_t>();
    q.nq = nq;
    const tcp_rx_acks acks(kConns);
    if (acks.workspace(n, nq) != sccsum_tcp_rx_acks_workspace(n, kConns, nq)) {
        std::printf("MISMATCH workspace\n");
        ++bad;
    }
    out_set a(kConns, acks.workspace(n, nq)), b(kConns, acks.workspace(n, nq));
    acks.run(rx, n, d_ack.as<sccsum_tcp_ack>(), q, kNow, a.out(), a.ws.p, stream);
    const tcp_rx_acks::outputs ob = b.out();
    const int rc = sccsum_tcp_rx_acks(rx.seg, rx.first, rx.run_conn, rx.run_first, rx.total, n, d_ack.as<sccsum_tcp_ack>(),
                                      kConns, q.first, q.len, q.meta, q.tx, nq, kNow, ob.run, ob.total, b.ws.p, stream);
    if (rc != SCCSUM_OK) {
        std::printf("sccsum_tcp_rx_acks: %s\n", sccsum_strerror(rc));
        return 2;
    }
    HIP_OK(hipStreamSynchronize(stream));
    same("run", a.run, b.run);
    same("total", a.total, b.total);
    uint64_t total[4];
    HIP_OK(hipMemcpy(total, a.total.p, sizeof(total), hipMemcpyDeviceToHost));
    std::vector<sccsum_tcp_ack_run> runs(kConns);
    HIP_OK(hipMemcpy(runs.data(), a.run.p, sizeof(sccsum_tcp_ack_run) * kConns, hipMemcpyDeviceToHost));
    uint64_t taken = 0, popped = 0, acked = 0;
    for (const sccsum_tcp_ack_run& r : runs) {
        taken += r.taken;
        popped += r.popped;
        acked += r.acked;
    }
    if (total[0] != kConns || total[1] != taken || total[2] != popped || total[3] != acked || taken < n0 / 2 ||
        taken >= n0 || popped == 0 || runs[13].stop != SCCSUM_TCP_STOP_INELIGIBLE || runs[21].stop != SCCSUM_TCP_STOP_QUEUE ||
        runs[7].taken != 1500 || runs[7].stop != SCCSUM_TCP_STOP_END || runs[5].una >= ack[5].una) {
        std::printf("MISMATCH total values: %llu runs, %llu taken, %llu popped, %llu acked\n",
                    static_cast<unsigned long long>(total[0]), static_cast<unsigned long long>(total[1]),
                    static_cast<unsigned long long>(total[2]), static_cast<unsigned long long>(total[3]));
        ++bad;
    }
    HIP_OK(hipStreamDestroy(stream));
    if (bad) return 1;
    std::printf("tcp_ack_gpu: OK (%llu records of %u connections: %llu taken, %llu entries popped)\n",
                static_cast<unsigned long long>(n0), kConns, static_cast<unsigned long long>(taken),
                static_cast<unsigned long long>(popped));
    return 0;
}
