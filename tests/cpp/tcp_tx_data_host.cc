// Stand-alone host program over seastar::net::tcp_tx_data
// (seastar/net/ip_checksum_batch.hh) and the C call it forwards to: workspace()
// and every argument error of sccsum_tcp_tx_data, which are all decided before
// any device work, so the program needs no GPU.  tests/test_tcp_tx_host.py
// builds it against the library and, with tcp_tx_data.hip compiled in, under
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
    sccsum_tcp_tx_opts opts{0x0A000001, 1500, 65535, 20, 0};
    bool no_opts = false;
    const sccsum_tcp_snd* snd = at<const sccsum_tcp_snd>(0x10000);
    uint32_t nconns = 4;
    const uint64_t* src = at<const uint64_t>(0x10000);
    const uint32_t* len = at<const uint32_t>(0x10000);
    const uint32_t* first = at<const uint32_t>(0x10000);
    uint64_t nbuf = 8;
    uint64_t max_segs = 64;
    uint64_t max_out_bytes = 1 << 20;
    sccsum_tcp_snd_run* run = at<sccsum_tcp_snd_run>(0x10000);
    uint64_t* off = at<uint64_t>(0x10000);
    uint32_t* out_len = at<uint32_t>(0x10000);
    sccsum_tcp_out* out = at<sccsum_tcp_out>(0x10000);
    uint32_t* seg_first = at<uint32_t>(0x10000);
    sccsum_gather_desc* desc = at<sccsum_gather_desc>(0x10000);
    uint64_t* total = at<uint64_t>(0x10000);
    void* ws = at<void>(0x10000);
};

int call(const args& a) {
    return sccsum_tcp_tx_data(a.no_opts ? nullptr : &a.opts, a.snd, a.nconns, a.src, a.len, a.first, a.nbuf, a.max_segs,
                              a.max_out_bytes, a.run, a.off, a.out_len, a.out, a.seg_first, a.desc, a.total, a.ws,
                              nullptr);
}

// The same through the class: true when run() throws.
bool throws(const args& a) {
    tcp_tx_data::queues q;
    q.src = a.src;
    q.len = a.len;
    q.first = a.first;
    q.nbuf = a.nbuf;
    tcp_tx_data::outputs out;
    out.run = a.run;
    out.off = a.off;
    out.len = a.out_len;
    out.out = a.out;
    out.seg_first = a.seg_first;
    out.desc = a.desc;
    out.total = a.total;
    try {
        tcp_tx_data(a.opts).run(a.snd, a.nconns, q, a.max_segs, a.max_out_bytes, out, a.ws, nullptr);
    } catch (const std::runtime_error&) {
        return true;
    }
    return false;
}

}  // namespace

int main() {
    static_assert(sizeof(sccsum_tcp_snd) == 48 && sizeof(sccsum_tcp_snd_run) == 32 && sizeof(sccsum_tcp_tx_opts) == 20,
                  "layout");
    static_assert(alignof(sccsum_tcp_snd) == 4 && offsetof(sccsum_tcp_snd, rcv_next) == 20 &&
                      offsetof(sccsum_tcp_snd, wnd) == 30 && offsetof(sccsum_tcp_snd, flags) == 32 &&
                      offsetof(sccsum_tcp_snd_run, next) == 12 && offsetof(sccsum_tcp_snd_run, stop) == 17,
                  "layout");
    const tcp_tx_data cut({1, 1500, 65535, 24, SCCSUM_TCP_TSO});
    expect(cut.opts().headroom == 24 && cut.opts().flags == SCCSUM_TCP_TSO, "opts");
    uint64_t before = 0;
    for (uint64_t nbuf : {uint64_t(0), uint64_t(1), uint64_t(1024), uint64_t(1025), uint64_t(1) << 20}) {
        const uint64_t w = tcp_tx_data::workspace(300, nbuf);
        expect(w == sccsum_tcp_tx_data_workspace(300, nbuf) && w % 16 == 0 && w > before, "workspace");
        before = w;
    }
    expect(tcp_tx_data::workspace(0, 0) != 0, "workspace of nothing");
    // per connection and per buffer, nothing per segment
    expect(tcp_tx_data::workspace(1 << 20, 1 << 20) < 40ull * (1 << 20) + 65536, "workspace is linear");
    expect(sccsum_tcp_tx_data_seg_tile() > 0 && sccsum_tcp_tx_data_max_blocks() > 0, "tile");

    // every call below is refused before any device work: the pointers are never followed
    std::vector<args> wrong;
    const auto add = [&](auto&& change) {
        args a;
        change(a);
        wrong.push_back(a);
    };
    add([](args& a) { a.opts.mtu = 67; });
    add([](args& a) { a.opts.mtu = 65536; });
    add([](args& a) { a.opts.headroom = 19; });
    add([](args& a) { a.opts.headroom = 65536; });
    add([](args& a) { a.opts.flags = SCCSUM_TCP_CSUM_OFFLOAD; });
    add([](args& a) { a.opts.flags = 0x80; });
    add([](args& a) { a.opts.flags = SCCSUM_TCP_TSO, a.opts.max_packet_len = 40; });
    add([](args& a) { a.opts.flags = SCCSUM_TCP_TSO, a.opts.max_packet_len = 65536; });
    add([](args& a) { a.snd = nullptr; });
    add([](args& a) { a.snd = at<const sccsum_tcp_snd>(0x10008); });
    add([](args& a) { a.src = nullptr; });
    add([](args& a) { a.src = at<const uint64_t>(0x10004); });
    add([](args& a) { a.len = nullptr; });
    add([](args& a) { a.len = at<const uint32_t>(0x10002); });
    add([](args& a) { a.first = nullptr; });
    add([](args& a) { a.first = at<const uint32_t>(0x10001); });
    add([](args& a) { a.run = nullptr; });
    add([](args& a) { a.run = at<sccsum_tcp_snd_run>(0x10008); });
    add([](args& a) { a.off = nullptr; });
    add([](args& a) { a.off = at<uint64_t>(0x10004); });
    add([](args& a) { a.out_len = nullptr; });
    add([](args& a) { a.out_len = at<uint32_t>(0x10002); });
    add([](args& a) { a.out = nullptr; });
    add([](args& a) { a.out = at<sccsum_tcp_out>(0x10002); });
    add([](args& a) { a.seg_first = nullptr; });
    add([](args& a) { a.seg_first = at<uint32_t>(0x10002); });
    add([](args& a) { a.desc = nullptr; });
    add([](args& a) { a.desc = at<sccsum_gather_desc>(0x10004); });
    add([](args& a) { a.total = nullptr; });
    add([](args& a) { a.total = at<uint64_t>(0x10004); });
    add([](args& a) { a.ws = nullptr; });
    add([](args& a) { a.ws = at<void>(0x10008); });
    add([](args& a) { a.nconns = SCCSUM_TCP_MAX_CONNS + 1; });
    add([](args& a) { a.nbuf = (uint64_t(1) << 31) + 1; });
    add([](args& a) { a.max_segs = uint64_t(1) << 31; });
    add([](args& a) { a.max_out_bytes = uint64_t(1) << 32; });
    add([](args& a) { a.nconns = 0, a.total = nullptr; });
    add([](args& a) { a.nconns = 0, a.seg_first = nullptr; });
    add([](args& a) { a.nconns = 0, a.ws = nullptr; });
    for (size_t k = 0; k < wrong.size(); ++k) {
        if (call(wrong[k]) != SCCSUM_EINVAL || !throws(wrong[k])) {
            std::printf("MISMATCH argument error %zu\n", k);
            ++bad;
        }
    }
    args none;
    none.no_opts = true;
    expect(call(none) == SCCSUM_EINVAL, "NULL opts");
    if (bad) return 1;
    std::printf("tcp_tx_data_host: OK (%zu argument errors)\n", wrong.size());
    return 0;
}
