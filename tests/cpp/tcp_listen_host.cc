// Stand-alone host program over seastar::net::tcp_listen
// (seastar/net/ip_checksum_batch.hh) and the C call it forwards to: workspace()
// and every argument error of sccsum_tcp_listen, which are all decided before
// any device work, so the program needs no GPU.  tests/test_tcp_listen_host.py
// builds it against the library and, with tcp_listen.hip compiled in, under
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
    sccsum_tcp_listen_opts opts{{1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, 77, 1500, 0};
    const void* bytes = at<const void>(0x10000);
    uint64_t bytes_len = 4096;
    const uint64_t* off = at<const uint64_t>(0x10000);
    uint64_t nbatch = 64;
    const uint32_t* first = at<const uint32_t>(0x10000);
    const uint32_t* order = at<const uint32_t>(0x10000);
    const sccsum_tcp_seg* seg = at<const sccsum_tcp_seg>(0x10000);
    const uint32_t* src = at<const uint32_t>(0x10000);
    uint64_t m_max = 64;
    const uint32_t* space = at<const uint32_t>(0x10000);
    uint8_t* cls = at<uint8_t>(0x10001);
    sccsum_tcp_new* rec = at<sccsum_tcp_new>(0x10000);
    void* synack = at<void>(0x10004);
    uint64_t* sa_off = at<uint64_t>(0x10008);
    uint32_t* sa_len = at<uint32_t>(0x10004);
    sccsum_tcp_out* sa_out = at<sccsum_tcp_out>(0x10004);
    void* rst = at<void>(0x10004);
    uint32_t* rst_dst = at<uint32_t>(0x10004);
    uint64_t* total = at<uint64_t>(0x10008);
    void* ws = at<void>(0x10000);
};

int call(const args& a) {
    return sccsum_tcp_listen(a.opts, a.bytes, a.bytes_len, a.off, a.nbatch, a.first, a.order, a.seg, a.src, a.m_max, a.space,
                             a.cls, a.rec, a.synack, a.sa_off, a.sa_len, a.sa_out, a.rst, a.rst_dst, a.total, a.ws,
                             nullptr);
}

// The same through the class: true when run() throws.
bool throws(const args& a) {
    device_packet_batch ip;
    ip.bytes = a.bytes;
    ip.bytes_len = a.bytes_len;
    ip.off = a.off;
    ip.n = a.nbatch;
    tcp_rx::outputs rx;
    rx.first = const_cast<uint32_t*>(a.first);
    rx.order = const_cast<uint32_t*>(a.order);
    rx.seg = const_cast<sccsum_tcp_seg*>(a.seg);
    rx.src = const_cast<uint32_t*>(a.src);
    tcp_listen::outputs out;
    out.cls = a.cls;
    out.rec = a.rec;
    out.synack = a.synack;
    out.sa_off = a.sa_off;
    out.sa_len = a.sa_len;
    out.sa_out = a.sa_out;
    out.rst = a.rst;
    out.rst_dst = a.rst_dst;
    out.total = a.total;
    try {
        tcp_listen(a.opts).run(ip, rx, a.m_max, a.space, out, a.ws, nullptr);
    } catch (const std::runtime_error&) {
        return true;
    }
    return false;
}

}  // namespace

int main() {
    static_assert(sizeof(sccsum_tcp_new) == 64 && sizeof(sccsum_tcp_listen_opts) == 76, "layout");
    static_assert(alignof(sccsum_tcp_new) == 4 && offsetof(sccsum_tcp_new, local_port) == 8 &&
                      offsetof(sccsum_tcp_new, pos) == 12 && offsetof(sccsum_tcp_new, iss) == 20 &&
                      offsetof(sccsum_tcp_new, cwnd) == 28 && offsetof(sccsum_tcp_new, rcv_window) == 36 &&
                      offsetof(sccsum_tcp_new, wl2) == 44 && offsetof(sccsum_tcp_new, snd_mss) == 48 &&
                      offsetof(sccsum_tcp_new, snd_wscale) == 52 && offsetof(sccsum_tcp_new, flags) == 54 &&
                      offsetof(sccsum_tcp_new, reserved) == 56 && offsetof(sccsum_tcp_listen_opts, isn_m) == 64 &&
                      offsetof(sccsum_tcp_listen_opts, mtu) == 68 && offsetof(sccsum_tcp_listen_opts, flags) == 72,
                  "layout");
    tcp_listen listen(args{}.opts);
    expect(listen.opts().mtu == 1500 && listen.opts().isn_m == 77 && listen.opts().isn_key[15] == 16, "opts");
    listen.set_isn_m(78);
    expect(listen.opts().isn_m == 78, "set_isn_m");
    uint64_t before = 0;
    for (uint64_t m : {uint64_t(0), uint64_t(1), uint64_t(1023), uint64_t(1025), uint64_t(1) << 20}) {
        const uint64_t w = tcp_listen::workspace(m);
        expect(w == sccsum_tcp_listen_workspace(m) && w % 16 == 0 && w > before, "workspace");
        before = w;
    }
    // the connids, two sort buffers, three position lists and a table of at most 4 m slots, the per-port words
    expect(tcp_listen::workspace(1 << 20) < 80ull * (1 << 20) + (1 << 20), "workspace is linear");
    expect(tcp_listen::workspace(uint64_t(SCCSUM_TCP_LISTEN_MAX) + 1) == 0, "workspace past the limit");

    // every call below is refused before any device work: the pointers are never followed
    std::vector<args> wrong;
    const auto add = [&](auto&& change) {
        args a;
        change(a);
        wrong.push_back(a);
    };
    add([](args& a) { a.bytes = nullptr; });
    add([](args& a) { a.off = nullptr; });
    add([](args& a) { a.off = at<const uint64_t>(0x10004); });
    add([](args& a) { a.first = nullptr; });
    add([](args& a) { a.first = at<const uint32_t>(0x10002); });
    add([](args& a) { a.order = nullptr; });
    add([](args& a) { a.order = at<const uint32_t>(0x10001); });
    add([](args& a) { a.seg = nullptr; });
    add([](args& a) { a.seg = at<const sccsum_tcp_seg>(0x10004); });
    add([](args& a) { a.src = nullptr; });
    add([](args& a) { a.src = at<const uint32_t>(0x10002); });
    add([](args& a) { a.space = nullptr; });
    add([](args& a) { a.space = at<const uint32_t>(0x10002); });
    add([](args& a) { a.cls = nullptr; });
    add([](args& a) { a.rec = nullptr; });
    add([](args& a) { a.rec = at<sccsum_tcp_new>(0x10008); });
    add([](args& a) { a.synack = nullptr; });
    add([](args& a) { a.synack = at<void>(0x10002); });
    add([](args& a) { a.sa_off = nullptr; });
    add([](args& a) { a.sa_off = at<uint64_t>(0x10004); });
    add([](args& a) { a.sa_len = nullptr; });
    add([](args& a) { a.sa_len = at<uint32_t>(0x10002); });
    add([](args& a) { a.sa_out = nullptr; });
    add([](args& a) { a.sa_out = at<sccsum_tcp_out>(0x10002); });
    add([](args& a) { a.rst = nullptr; });
    add([](args& a) { a.rst = at<void>(0x10001); });
    add([](args& a) { a.rst_dst = nullptr; });
    add([](args& a) { a.rst_dst = at<uint32_t>(0x10002); });
    add([](args& a) { a.total = nullptr; });
    add([](args& a) { a.total = at<uint64_t>(0x10004); });
    add([](args& a) { a.ws = nullptr; });
    add([](args& a) { a.ws = at<void>(0x10008); });
    add([](args& a) { a.m_max = uint64_t(SCCSUM_TCP_LISTEN_MAX) + 1; });
    add([](args& a) { a.nbatch = uint64_t(1) << 32; });
    add([](args& a) { a.opts.mtu = 67; });
    add([](args& a) { a.opts.mtu = 65536; });
    add([](args& a) { a.opts.flags = SCCSUM_TCP_TSO; });
    add([](args& a) { a.opts.flags = 4; });
    add([](args& a) { a.m_max = 0, a.total = nullptr; });
    add([](args& a) { a.m_max = 0, a.ws = nullptr; });
    add([](args& a) { a.m_max = 0, a.opts.mtu = 0; });
    for (size_t k = 0; k < wrong.size(); ++k) {
        if (call(wrong[k]) != SCCSUM_EINVAL || !throws(wrong[k])) {
            std::printf("MISMATCH argument error %zu\n", k);
            ++bad;
        }
    }
    if (bad) return 1;
    std::printf("tcp_listen_host: OK (%zu argument errors)\n", wrong.size());
    return 0;
}
