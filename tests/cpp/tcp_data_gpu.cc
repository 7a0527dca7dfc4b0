// Native host program over the C++ class tcp_rx_data
// (seastar/net/ip_checksum_batch.hh): run() forwards 15 arguments, many of one
// type, five of them taken from tcp_rx's outputs struct, to a C call that the
// Python tests pin.  Here the wrapper and the C call run on the same inputs
// into two separately poisoned sets of outputs (64 guard bytes behind each
// array, the workspaces poisoned too), and every array must be byte-equal: a
// swapped or dropped argument, or a field mapped to the wrong parameter,
// shows.  The input is written as tcp_rx leaves it: two tiles + 300 records
// of 97 connections in runs of mixed length, most in sequence, some leaving
// the straight path (a gap, a FIN, a pure ACK, a new ACK), one connection not
// eligible, and a capacity that cuts the last runs off.
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
    dev_array run, desc, total, ws;
    out_set(uint64_t n, uint64_t runs, uint64_t ws_bytes)
        : run(sizeof(sccsum_tcp_rcv_run) * runs), desc(sizeof(sccsum_gather_desc) * n), total(8 * 4), ws(ws_bytes, 0x5A) {}
    tcp_rx_data::outputs out() const {
        tcp_rx_data::outputs o;
        o.run = run.as<sccsum_tcp_rcv_run>();
        o.desc = desc.as<sccsum_gather_desc>();
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
    std::mt19937 rng(83);

    constexpr uint32_t kConns = 97, kOthers = 11;
    const uint64_t n0 = 2 * uint64_t(sccsum_eth_tile_packets()) + 300, n = n0 + kOthers;
    std::vector<sccsum_tcp_rcv> rcv(kConns);
    std::vector<sccsum_tcp_seg> seg(n);
    std::vector<uint32_t> run_conn(kConns + 1), run_first(kConns + 1);
    uint64_t p = 0, pay = 0;
    for (uint32_t c = 0; c < kConns; ++c) {
        sccsum_tcp_rcv& s = rcv[c];
        s = sccsum_tcp_rcv{};
        s.next = static_cast<uint32_t>(rng());
        s.room = c == 40 ? 5000 : 1u << 22;
        s.cap = 29200u << 3;
        s.window = s.room < s.cap ? s.room : s.cap;
        s.snd_una = static_cast<uint32_t>(rng());
        s.mss = 1460;
        s.flags = static_cast<uint8_t>((c == 13 ? 0 : SCCSUM_TCP_RCV_ELIGIBLE) | (c & 1 ? SCCSUM_TCP_RCV_NR_FULL : 0) |
                                       (c & 2 ? SCCSUM_TCP_RCV_ACK_ARMED : 0));
        run_conn[c] = c;
        run_first[c] = static_cast<uint32_t>(p);
        const uint64_t count = c + 1 == kConns ? n0 - p : (c == 7 ? 1500 : 1 + rng() % 8);
        uint32_t seq = s.next;
        for (uint64_t k = 0; k < count; ++k, ++p) {
            sccsum_tcp_seg& g = seg[p];
            g = sccsum_tcp_seg{};
            g.pay_len = (k % 3 == 0) ? 1460 : 1 + rng() % 2000;
            g.pay_off = pay;
            pay += g.pay_len + k % 4;
            g.seq = seq;
            g.ack = s.snd_una;
            g.conn = c;
            g.flags = 0x10 | (k % 5 == 0 ? 0x08 : 0);
            g.hdr_len = 20;
            if (c % 9 == 3 && k == 4) g.seq += 100;              // a gap
            if (c % 9 == 4 && k == 2) g.flags |= 0x01;           // FIN
            if (c % 9 == 5 && k == 3) g.pay_len = 0;             // a pure ACK
            if (c % 9 == 6 && k == 1) g.ack += 1;                // a new ACK
            seq += g.pay_len;
        }
    }
    run_first[kConns] = static_cast<uint32_t>(n0);
    for (uint64_t k = n0; k < n; ++k) {
        seg[k] = sccsum_tcp_seg{};
        seg[k].conn = UINT32_MAX;
        seg[k].pay_len = 77;
    }
    const std::vector<uint32_t> first = {0, static_cast<uint32_t>(n0), static_cast<uint32_t>(n0 + 4),
                                         static_cast<uint32_t>(n), static_cast<uint32_t>(n)};
    const std::vector<uint64_t> rx_total = {kConns, kOthers - 4, 0, 0};
    dev_array d_seg(sizeof(sccsum_tcp_seg) * n), d_rcv(sizeof(sccsum_tcp_rcv) * kConns), d_first(4 * 5),
        d_run_conn(4 * (kConns + 1)), d_run_first(4 * (kConns + 1)), d_rx_total(8 * 4), d_bytes(256);
    upload(d_seg, seg);
    upload(d_rcv, rcv);
    upload(d_first, first);
    upload(d_run_conn, run_conn);
    upload(d_run_first, run_first);
    upload(d_rx_total, rx_total);

    tcp_rx::outputs rx;
    rx.seg = d_seg.as<sccsum_tcp_seg>();
    rx.first = d_first.as<uint32_t>();
    rx.run_conn = d_run_conn.as<uint32_t>();
    rx.run_first = d_run_first.as<uint32_t>();
    rx.total = d_rx_total.as<uint64_t>();
    const tcp_rx_data data(kConns);
    if (data.workspace(n) != sccsum_tcp_rx_data_workspace(n, kConns)) {
        std::printf("MISMATCH workspace\n");
        ++bad;
    }
    uint64_t needed = 0, emitted[2] = {0, 0};
    for (int round = 0; round < 2; ++round) {
        // the second round with a capacity that cuts the last runs off
        const uint64_t max_bytes = round == 0 ? 0xFFFFFFFFull : needed - 1000;
        out_set a(n, kConns + 1, data.workspace(n)), b(n, kConns + 1, data.workspace(n));
        data.run(d_bytes.p, rx, n, d_rcv.as<sccsum_tcp_rcv>(), max_bytes, a.out(), a.ws.p, stream);
        const tcp_rx_data::outputs ob = b.out();
        const int rc = sccsum_tcp_rx_data(d_bytes.p, rx.seg, rx.first, rx.run_conn, rx.run_first, rx.total, n,
                                          d_rcv.as<sccsum_tcp_rcv>(), kConns, max_bytes, ob.run, ob.desc, ob.total, b.ws.p,
                                          stream);
        if (rc != SCCSUM_OK) {
            std::printf("sccsum_tcp_rx_data: %s\n", sccsum_strerror(rc));
            return 2;
        }
        HIP_OK(hipStreamSynchronize(stream));
        same("run", a.run, b.run);
        same("desc", a.desc, b.desc);
        same("total", a.total, b.total);
        uint64_t total[4];
        HIP_OK(hipMemcpy(total, a.total.p, sizeof(total), hipMemcpyDeviceToHost));
        std::vector<sccsum_tcp_rcv_run> runs(kConns);
        HIP_OK(hipMemcpy(runs.data(), a.run.p, sizeof(sccsum_tcp_rcv_run) * kConns, hipMemcpyDeviceToHost));
        uint64_t taken = 0, bytes = 0, cut = 0;
        for (const sccsum_tcp_rcv_run& r : runs) {
            if (r.desc_first != taken || r.dst_off != bytes) {
                std::printf("MISMATCH run.desc_first / dst_off\n");
                ++bad;
                break;
            }
            taken += r.taken;
            bytes += r.bytes;
            cut += r.stop == SCCSUM_TCP_STOP_CAPACITY;
        }
        if (total[0] != taken || total[1] != bytes || total[3] != 0 || taken < n0 / 2 || taken >= n0 ||
            runs[13].stop != SCCSUM_TCP_STOP_INELIGIBLE || runs[7].taken != 1500 || (round == 0) != (cut == 0) ||
            (round == 0 ? total[2] != bytes : total[2] != needed || bytes > max_bytes)) {
            std::printf("MISMATCH total values: %llu taken, %llu bytes, %llu needed, %llu runs cut\n",
                        static_cast<unsigned long long>(total[0]), static_cast<unsigned long long>(total[1]),
                        static_cast<unsigned long long>(total[2]), static_cast<unsigned long long>(cut));
            ++bad;
        }
        needed = total[2];
        emitted[round] = total[0];
    }
    HIP_OK(hipStreamDestroy(stream));
    if (bad) return 1;
    std::printf("tcp_data_gpu: OK (%llu records of %u connections: %llu taken, %llu under the capacity)\n",
                static_cast<unsigned long long>(n0), kConns, static_cast<unsigned long long>(emitted[0]),
                static_cast<unsigned long long>(emitted[1]));
    return 0;
}
