// Stand-alone host program over seastar::net::tcp_rx_acks
// (seastar/net/ip_checksum_batch.hh) and the C call it forwards to: workspace()
// and every argument error of sccsum_tcp_rx_acks, which are all decided before
// any device work, so the program needs no GPU.  tests/test_tcp_ack_host.py
// builds it against the library and, with tcp_ack.hip compiled in, under
// AddressSanitizer + UndefinedBehaviorSanitizer on the host code.
// Prints OK and exits 0; a mismatch prints what differed and exits 1.
#include <seastar/net/ip_checksum_batch.hh>

#include <cstddef>
#include <cstdio>
#include <stdexcept>
#include <vector>

using namespace seastar::net;

namespace {

int bad = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("MISMATCH %s\n", what);
        ++bad;
    }
}

template <typename T>
T* at(uintptr_t p) {
    return reinterpret_cast<T*>(p);
}

struct args {
    const sccsum_tcp_seg* seg = at<const sccsum_tcp_seg>(0x10000);
    const uint32_t* first = at<const uint32_t>(0x10000);
    const uint32_t* run_conn = at<const uint32_t>(0x10000);
    const uint32_t* run_first = at<const uint32_t>(0x10000);
    const uint64_t* rx_total = at<const uint64_t>(0x10000);
    uint64_t n = 64;
    const sccsum_tcp_ack* ack = at<const sccsum_tcp_ack>(0x10000);
    uint32_t nconns = 4;
    const uint32_t* q_first = at<const uint32_t>(0x10000);
    const uint32_t* q_len = at<const uint32_t>(0x10000);
    const uint32_t* q_meta = at<const uint32_t>(0x10000);
    const int64_t* q_tx = at<const int64_t>(0x10000);
    uint64_t nq = 8;
    sccsum_tcp_ack_run* run = at<sccsum_tcp_ack_run>(0x10000);
    uint64_t* total = at<uint64_t>(0x10000);
    void* ws = at<void>(0x10000);
};

int call(const args& a) {
    return sccsum_tcp_rx_acks(a.seg, a.first, a.run_conn, a.run_first, a.rx_total, a.n, a.ack, a.nconns, a.q_first, a.q_len,
                              a.q_meta, a.q_tx, a.nq, 12345, a.run, a.total, a.ws, nullptr);
}

// The same through the class: true when run() throws.
bool throws(const args& a) {
    tcp_rx::outputs rx;
    rx.seg = const_cast<sccsum_tcp_seg*>(a.seg);
    rx.first = const_cast<uint32_t*>(a.first);
    rx.run_conn = const_cast<uint32_t*>(a.run_conn);
    rx.run_first = const_cast<uint32_t*>(a.run_first);
    rx.total = const_cast<uint64_t*>(a.rx_total);
    tcp_rx_acks::queues q;
    q.first = a.q_first;
    q.len = a.q_len;
    q.meta = a.q_meta;
    q.tx = a.q_tx;
    q.nq = a.nq;
    tcp_rx_acks::outputs out;
    out.run = a.run;
    out.total = a.total;
    try {
        tcp_rx_acks(a.nconns).run(rx, a.n, a.ack, q, 12345, out, a.ws, nullptr);
    } catch (const std::runtime_error&) {
        return true;
    }
    return false;
}

}  // namespace

int main() {
    static_assert(sizeof(sccsum_tcp_ack) == 64 && sizeof(sccsum_tcp_ack_run) == 64, "layout");
    static_assert(alignof(sccsum_tcp_ack) == 8 && offsetof(sccsum_tcp_ack, unsent_len) == 28 &&
                      offsetof(sccsum_tcp_ack, rto) == 36 && offsetof(sccsum_tcp_ack, srtt) == 40 &&
                      offsetof(sccsum_tcp_ack, window_scale) == 58 && offsetof(sccsum_tcp_ack, flags) == 59 &&
                      offsetof(sccsum_tcp_ack_run, cwnd) == 28 && offsetof(sccsum_tcp_ack_run, rttvar) == 40 &&
                      offsetof(sccsum_tcp_ack_run, rto) == 48 && offsetof(sccsum_tcp_ack_run, stop) == 53,
                  "layout");
    const tcp_rx_acks acks(300);
    expect(acks.nconns() == 300, "nconns");
    uint64_t before = 0;
    for (uint64_t nq : {uint64_t(0), uint64_t(1), uint64_t(1024), uint64_t(1025), uint64_t(1) << 20}) {
        const uint64_t w = acks.workspace(5000, nq);
        expect(w == sccsum_tcp_rx_acks_workspace(5000, 300, nq) && w % 16 == 0 && w > before, "workspace");
        before = w;
    }
    expect(tcp_rx_acks(0).workspace(0, 0) != 0, "workspace of nothing");
    // a pair per record, two scans per entry, three sums per block of runs
    expect(tcp_rx_acks(1 << 20).workspace(1 << 20, 1 << 20) < 24ull * (1 << 20) + 65536, "workspace is linear");

    // every call below is refused before any device work: the pointers are never followed
    std::vector<args> wrong;
    const auto add = [&](auto&& change) {
        args a;
        change(a);
        wrong.push_back(a);
    };
    add([](args& a) { a.seg = nullptr; });
    add([](args& a) { a.seg = at<const sccsum_tcp_seg>(0x10004); });
    add([](args& a) { a.first = nullptr; });
    add([](args& a) { a.first = at<const uint32_t>(0x10002); });
    add([](args& a) { a.run_conn = nullptr; });
    add([](args& a) { a.run_conn = at<const uint32_t>(0x10001); });
    add([](args& a) { a.run_first = nullptr; });
    add([](args& a) { a.run_first = at<const uint32_t>(0x10002); });
    add([](args& a) { a.rx_total = nullptr; });
    add([](args& a) { a.rx_total = at<const uint64_t>(0x10004); });
    add([](args& a) { a.ack = nullptr; });
    add([](args& a) { a.ack = at<const sccsum_tcp_ack>(0x10008); });
    add([](args& a) { a.q_first = nullptr; });
    add([](args& a) { a.q_first = at<const uint32_t>(0x10002); });
    add([](args& a) { a.q_len = nullptr; });
    add([](args& a) { a.q_len = at<const uint32_t>(0x10002); });
    add([](args& a) { a.q_meta = nullptr; });
    add([](args& a) { a.q_meta = at<const uint32_t>(0x10001); });
    add([](args& a) { a.q_tx = nullptr; });
    add([](args& a) { a.q_tx = at<const int64_t>(0x10004); });
    add([](args& a) { a.run = nullptr; });
    add([](args& a) { a.run = at<sccsum_tcp_ack_run>(0x10008); });
    add([](args& a) { a.total = nullptr; });
    add([](args& a) { a.total = at<uint64_t>(0x10004); });
    add([](args& a) { a.ws = nullptr; });
    add([](args& a) { a.ws = at<void>(0x10008); });
    add([](args& a) { a.n = uint64_t(1) << 32; });
    add([](args& a) { a.nconns = SCCSUM_TCP_MAX_CONNS + 1; });
    add([](args& a) { a.nq = (uint64_t(1) << 31) + 1; });
    add([](args& a) { a.n = 0, a.total = nullptr; });
    add([](args& a) { a.n = 0, a.ws = nullptr; });
    add([](args& a) { a.n = 0, a.q_first = nullptr; });
    for (size_t k = 0; k < wrong.size(); ++k) {
        if (call(wrong[k]) != SCCSUM_EINVAL || !throws(wrong[k])) {
            std::printf("MISMATCH argument error %zu\n", k);
            ++bad;
        }
    }
    if (bad) return 1;
    std::printf("tcp_ack_host: OK (%zu argument errors)\n", wrong.size());
    return 0;
}
