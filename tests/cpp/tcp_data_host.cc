// Stand-alone host program over seastar::net::tcp_rx_data
// (seastar/net/ip_checksum_batch.hh) and the C call it forwards to: workspace()
// and every argument error of sccsum_tcp_rx_data, which are all decided before
// any device work, so the program needs no GPU.  tests/test_tcp_data_host.py
// builds it against the library and, with tcp_data.hip compiled in, under
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

struct args {
    const void* bytes = reinterpret_cast<const void*>(0x10000);
    const sccsum_tcp_seg* seg = reinterpret_cast<const sccsum_tcp_seg*>(0x10000);
    const uint32_t* first = reinterpret_cast<const uint32_t*>(0x10000);
    const uint32_t* run_conn = reinterpret_cast<const uint32_t*>(0x10000);
    const uint32_t* run_first = reinterpret_cast<const uint32_t*>(0x10000);
    const uint64_t* rx_total = reinterpret_cast<const uint64_t*>(0x10000);
    uint64_t n = 8;
    const sccsum_tcp_rcv* rcv = reinterpret_cast<const sccsum_tcp_rcv*>(0x10000);
    uint32_t nconns = 4;
    uint64_t max_bytes = 1 << 20;
    sccsum_tcp_rcv_run* run = reinterpret_cast<sccsum_tcp_rcv_run*>(0x10000);
    sccsum_gather_desc* desc = reinterpret_cast<sccsum_gather_desc*>(0x10000);
    uint64_t* total = reinterpret_cast<uint64_t*>(0x10000);
    void* ws = reinterpret_cast<void*>(0x10000);
};

int call(const args& a) {
    return sccsum_tcp_rx_data(a.bytes, a.seg, a.first, a.run_conn, a.run_first, a.rx_total, a.n, a.rcv, a.nconns,
                              a.max_bytes, a.run, a.desc, a.total, a.ws, nullptr);
}

// The same through the class: true when run() throws.
bool throws(const args& a) {
    tcp_rx::outputs rx;
    rx.seg = const_cast<sccsum_tcp_seg*>(a.seg);
    rx.first = const_cast<uint32_t*>(a.first);
    rx.run_conn = const_cast<uint32_t*>(a.run_conn);
    rx.run_first = const_cast<uint32_t*>(a.run_first);
    rx.total = const_cast<uint64_t*>(a.rx_total);
    tcp_rx_data::outputs out;
    out.run = a.run;
    out.desc = a.desc;
    out.total = a.total;
    try {
        tcp_rx_data(a.nconns).run(a.bytes, rx, a.n, a.rcv, a.max_bytes, out, a.ws, nullptr);
    } catch (const std::runtime_error&) {
        return true;
    }
    return false;
}

template <typename T>
T* at(uintptr_t p) {
    return reinterpret_cast<T*>(p);
}

}  // namespace

int main() {
    static_assert(sizeof(sccsum_tcp_rcv) == 32 && sizeof(sccsum_tcp_rcv_run) == 32, "layout");
    static_assert(alignof(sccsum_tcp_rcv) == 4 && offsetof(sccsum_tcp_rcv, mss) == 20 &&
                      offsetof(sccsum_tcp_rcv, flags) == 22 && offsetof(sccsum_tcp_rcv_run, flags) == 28 &&
                      offsetof(sccsum_tcp_rcv_run, stop) == 29,
                  "layout");
    const tcp_rx_data data(300);
    expect(data.nconns() == 300, "nconns");
    for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(1024), uint64_t(1025), uint64_t(1) << 20}) {
        expect(data.workspace(n) == sccsum_tcp_rx_data_workspace(n, 300) && data.workspace(n) % 16 == 0 &&
                   data.workspace(n) != 0,
               "workspace");
    }
    expect(data.workspace(1 << 20) < (1 << 20), "workspace is per tile");

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
    add([](args& a) { a.run_conn = at<const uint32_t>(0x10002); });
    add([](args& a) { a.run_first = nullptr; });
    add([](args& a) { a.run_first = at<const uint32_t>(0x10001); });
    add([](args& a) { a.rx_total = nullptr; });
    add([](args& a) { a.rx_total = at<const uint64_t>(0x10004); });
    add([](args& a) { a.rcv = nullptr; });
    add([](args& a) { a.rcv = at<const sccsum_tcp_rcv>(0x10008); });
    add([](args& a) { a.run = nullptr; });
    add([](args& a) { a.run = at<sccsum_tcp_rcv_run>(0x10004); });
    add([](args& a) { a.desc = nullptr; });
    add([](args& a) { a.desc = at<sccsum_gather_desc>(0x10004); });
    add([](args& a) { a.total = nullptr; });
    add([](args& a) { a.total = at<uint64_t>(0x10004); });
    add([](args& a) { a.ws = nullptr; });
    add([](args& a) { a.ws = at<void>(0x10008); });
    add([](args& a) { a.n = uint64_t(1) << 32; });
    add([](args& a) { a.nconns = SCCSUM_TCP_MAX_CONNS + 1; });
    add([](args& a) { a.max_bytes = uint64_t(1) << 32; });
    add([](args& a) { a.n = 0, a.total = nullptr; });
    add([](args& a) { a.n = 0, a.ws = nullptr; });
    for (size_t k = 0; k < wrong.size(); ++k) {
        if (call(wrong[k]) != SCCSUM_EINVAL || !throws(wrong[k])) {
            std::printf("MISMATCH argument error %zu\n", k);
            ++bad;
        }
    }
    if (bad) return 1;
    std::printf("tcp_data_host: OK (%zu argument errors)\n", wrong.size());
    return 0;
}
