// Native host program over the C++ class tcp_listen
// (seastar/net/ip_checksum_batch.hh): run() forwards 22 arguments, many of one
// type, four of them taken from the batch, four from tcp_rx's outputs struct
// and nine from its own, to a C call that the Python tests pin.  Here the
// wrapper and the C call run on the same inputs into two separately poisoned
// sets of outputs (64 guard bytes behind each array, the workspaces poisoned
// too), and every array must be byte-equal: a swapped or dropped argument, or
// a field mapped to the wrong parameter, shows.  The input is written as
// tcp_rx leaves it: a LISTEN bucket of 2 100 segments between two others, SYNs
// of distinct peers with MSS and window-scale options to three ports of which
// one fills, ACKs and RSTs among them, and near the end a second SYN of a
// created connection.  The counts are checked against what the program itself
// put in.
// Prints OK and exits 0; a mismatch prints the array's name and exits 1.
#include <hip/hip_runtime.h>
#include <seastar/net/ip_checksum_batch.hh>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    dev_array cls, rec, synack, sa_off, sa_len, sa_out, rst, rst_dst, total, ws;
    out_set(uint64_t m, uint64_t ws_bytes)
        : cls(m), rec(sizeof(sccsum_tcp_new) * m), synack(32 * m), sa_off(8 * m), sa_len(4 * m),
          sa_out(sizeof(sccsum_tcp_out) * m), rst(20 * m), rst_dst(4 * m), total(8 * 4), ws(ws_bytes, 0x5A) {}
    tcp_listen::outputs out() const {
        tcp_listen::outputs o;
        o.cls = cls.as<uint8_t>();
        o.rec = rec.as<sccsum_tcp_new>();
        o.synack = synack.p;
        o.sa_off = sa_off.as<uint64_t>();
        o.sa_len = sa_len.as<uint32_t>();
        o.sa_out = sa_out.as<sccsum_tcp_out>();
        o.rst = rst.p;
        o.rst_dst = rst_dst.as<uint32_t>();
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

    constexpr uint32_t kLead = 5, kTrail = 3, kM = 2100, kHost = 0x0A000001, kPeer = 0x0A000110;
    constexpr uint32_t kFrame = 20 + 28;                 // an IPv4 header, a TCP header with eight option bytes
    constexpr uint32_t kRoom = 700, kStop = 2000;        // port 81 has room for 700; position 2000 repeats position 0
    const uint64_t n = kLead + kM + kTrail;
    std::vector<uint8_t> bytes(n * kFrame + 16, 0);
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> order(n), src(n), first{0, kLead, kLead + kM, uint32_t(n), uint32_t(n)};
    std::vector<sccsum_tcp_seg> seg(n);
    uint64_t syn81 = 0, want_new = 0, want_rst = 0, want_drop = 0;
    for (uint64_t p = 0; p < n; ++p) {
        const uint64_t frame = (p * 7) % n;              // 7 and n = 2108 are coprime: the frames lie in another order
        order[p] = static_cast<uint32_t>(frame);
        off[frame] = frame * kFrame;
        uint8_t* const ip = bytes.data() + off[frame];
        ip[0] = 0x45;
        ip[16] = kHost >> 24, ip[17] = (kHost >> 16) & 0xFF, ip[18] = (kHost >> 8) & 0xFF, ip[19] = kHost & 0xFF;
        const uint8_t opt[8] = {2, 4, 0x05, 0xB4, 3, 3, uint8_t(p % 15), 0};
        std::memcpy(ip + 40, opt, 8);
        const uint64_t i = p - kLead;                    // the position in the bucket
        const bool in_bucket = p >= kLead && p < kLead + kM;
        const uint64_t peer = in_bucket && i == kStop ? 0 : i;
        sccsum_tcp_seg s{};
        s.pay_off = off[frame] + kFrame;
        s.seq = static_cast<uint32_t>(1000 + peer);
        s.ack = static_cast<uint32_t>(peer * 3);
        s.conn = in_bucket ? UINT32_MAX : 0;
        s.window = static_cast<uint16_t>(100 + peer);
        s.sport = static_cast<uint16_t>(1024 + peer % 50000);
        s.dport = static_cast<uint16_t>(80 + peer % 3);
        s.flags = i % 11 == 5 ? 0x10 : i % 13 == 7 ? 0x04 : 0x02;
        s.hdr_len = 28;
        seg[p] = s;
        src[p] = kPeer + static_cast<uint32_t>(peer / 50000);
        if (in_bucket && i < kStop) {
            const bool full = s.dport == 82 || (s.dport == 81 && syn81 >= kRoom);
            if (s.flags == 0x04) {
                ++want_drop;
            } else if (full || s.flags == 0x10) {
                ++want_rst;
            } else {
                ++want_new;
                if (s.dport == 81) ++syn81;
            }
        }
    }
    std::vector<uint32_t> space(65536, 0);
    space[80] = 1u << 20;
    space[81] = kRoom;

    dev_array d_bytes(bytes.size()), d_off(8 * n), d_order(4 * n), d_src(4 * n), d_first(4 * 5), d_seg(sizeof(sccsum_tcp_seg) * n),
        d_space(4 * 65536);
    upload(d_bytes, bytes);
    upload(d_off, off);
    upload(d_order, order);
    upload(d_src, src);
    upload(d_first, first);
    upload(d_seg, seg);
    upload(d_space, space);

    sccsum_tcp_listen_opts opts{};
    for (uint32_t k = 0; k < 16; ++k) opts.isn_key[k] = 0x01010101u * k + 7;
    opts.isn_m = 0xFFFF0000u;
    opts.mtu = 1500;
    opts.flags = SCCSUM_TCP_CSUM_OFFLOAD;
    const tcp_listen listen(opts);
    const uint64_t m_max = kM + 9;                       // a bound, not the size
    const uint64_t ws_bytes = tcp_listen::workspace(m_max);
    out_set a(m_max, ws_bytes), b(m_max, ws_bytes);

    device_packet_batch ip;
    ip.bytes = d_bytes.p;
    ip.bytes_len = n * kFrame;
    ip.off = d_off.as<uint64_t>();
    ip.n = n;
    tcp_rx::outputs rx;
    rx.first = d_first.as<uint32_t>();
    rx.order = d_order.as<uint32_t>();
    rx.seg = d_seg.as<sccsum_tcp_seg>();
    rx.src = d_src.as<uint32_t>();
    listen.run(ip, rx, m_max, d_space.as<uint32_t>(), a.out(), a.ws.p, stream);
    const tcp_listen::outputs o = b.out();
    const int rc = sccsum_tcp_listen(opts, d_bytes.p, n * kFrame, d_off.as<uint64_t>(), n, d_first.as<uint32_t>(),
                                     d_order.as<uint32_t>(), d_seg.as<sccsum_tcp_seg>(), d_src.as<uint32_t>(), m_max,
                                     d_space.as<uint32_t>(), o.cls, o.rec, o.synack, o.sa_off, o.sa_len, o.sa_out, o.rst,
                                     o.rst_dst, o.total, b.ws.p, stream);
    if (rc != SCCSUM_OK) {
        std::printf("sccsum_tcp_listen: %s\n", sccsum_strerror(rc));
        return 1;
    }
    HIP_OK(hipStreamSynchronize(stream));

    same("cls", a.cls, b.cls);
    same("rec", a.rec, b.rec);
    same("synack", a.synack, b.synack);
    same("sa_off", a.sa_off, b.sa_off);
    same("sa_len", a.sa_len, b.sa_len);
    same("sa_out", a.sa_out, b.sa_out);
    same("rst", a.rst, b.rst);
    same("rst_dst", a.rst_dst, b.rst_dst);
    same("total", a.total, b.total);

    uint64_t total[4];
    HIP_OK(hipMemcpy(total, a.total.p, sizeof(total), hipMemcpyDeviceToHost));
    if (total[0] != kStop || total[1] != want_new || total[2] != want_rst || total[3] != want_drop) {
        std::printf("MISMATCH total {%llu, %llu, %llu, %llu}, expected {%u, %llu, %llu, %llu}\n",
                    static_cast<unsigned long long>(total[0]), static_cast<unsigned long long>(total[1]),
                    static_cast<unsigned long long>(total[2]), static_cast<unsigned long long>(total[3]), kStop,
                    static_cast<unsigned long long>(want_new), static_cast<unsigned long long>(want_rst),
                    static_cast<unsigned long long>(want_drop));
        ++bad;
    }
    std::vector<sccsum_tcp_new> rec(want_new);
    HIP_OK(hipMemcpy(rec.data(), a.rec.p, rec.size() * sizeof(sccsum_tcp_new), hipMemcpyDeviceToHost));
    const sccsum_tcp_new& r0 = rec[0];
    if (r0.pos != 0 || r0.local_ip != kHost || r0.foreign_ip != kPeer || r0.local_port != 80 || r0.foreign_port != 1024 ||
        r0.irs != 1000 || r0.snd_mss != 1460 || r0.local_mss != 1460 || r0.rcv_wscale != 7 || r0.cwnd != 3 * 1460 ||
        r0.flags != (SCCSUM_TCP_NEW_MSS | SCCSUM_TCP_NEW_WSCALE)) {
        std::printf("MISMATCH the first record\n");
        ++bad;
    }
    HIP_OK(hipStreamDestroy(stream));
    if (bad) return 1;
    std::printf("tcp_listen_gpu: OK (%llu created, %llu resets, %llu dropped of %u before the stop)\n",
                static_cast<unsigned long long>(want_new), static_cast<unsigned long long>(want_rst),
                static_cast<unsigned long long>(want_drop), kStop);
    return 0;
}
