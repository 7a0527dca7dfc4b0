// Native host program over the C++ classes udp_ports, udp_rx and udp_tx
// (seastar/net/ip_checksum_batch.hh): each forwards a dozen or more arguments,
// many of one type, to a C call that the Python tests pin.  Here the wrapper
// and the C call it forwards to run on the same inputs into two separately
// poisoned sets of outputs (64 guard bytes behind each array, the workspaces
// poisoned too), every optional argument given, and every array must be
// byte-equal: a swapped or dropped argument shows.  The inputs span a tile
// edge: a tile + 300 IPv4 packets (UDP to bound and unbound ports, short ones,
// TCP) through udp_rx::run with an index, the same packets' L4 parts as
// two-descriptor datagrams through udp_rx::run_reassembled, and their payloads
// through udp_tx::run on two copies of the buffer.
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

void c_ok(int rc, const char* what) {
    if (rc != SCCSUM_OK) {
        std::printf("%s: %s\n", what, sccsum_strerror(rc));
        std::exit(2);
    }
}

struct rx_set {
    dev_array cls, first, order, pay_off, pay_len, src, sport, ws;
    rx_set(uint64_t n, uint32_t channels)
        : cls(n), first(4 * (channels + 2)), order(4 * n), pay_off(8 * n), pay_len(4 * n), src(4 * n), sport(2 * n),
          ws(udp_rx::workspace(n), 0x5A) {}
    udp_rx::outputs out() const {
        return udp_rx::outputs{cls.as<uint8_t>(),      first.as<uint32_t>(), order.as<uint32_t>(), pay_off.as<uint64_t>(),
                               pay_len.as<uint32_t>(), src.as<uint32_t>(),   sport.as<uint16_t>()};
    }
    void compare(const char* what, const rx_set& o, bool with_off) const {
        char name[64];
        const struct {
            const char* n;
            const dev_array *a, *b;
        } all[] = {{"cls", &cls, &o.cls},       {"first", &first, &o.first},       {"order", &order, &o.order},
                   {"pay_off", &pay_off, &o.pay_off}, {"pay_len", &pay_len, &o.pay_len}, {"src", &src, &o.src},
                   {"sport", &sport, &o.sport}};
        for (const auto& e : all) {
            if (!with_off && e.a == &pay_off) continue;
            std::snprintf(name, sizeof(name), "%s.%s", what, e.n);
            same(name, *e.a, *e.b);
        }
    }
};

struct tx_set {
    dev_array bytes, l4_off, l4_len, sum_len, seed, proto, needs_csum, status;
    tx_set(size_t nbytes, uint64_t n)
        : bytes(nbytes), l4_off(8 * n), l4_len(4 * n), sum_len(4 * n), seed(4 * n), proto(n), needs_csum(n), status(n) {}
    udp_tx::outputs out() const {
        return udp_tx::outputs{l4_off.as<uint64_t>(), l4_len.as<uint32_t>(), sum_len.as<uint32_t>(), seed.as<uint32_t>(),
                               proto.as<uint8_t>(),   needs_csum.as<uint8_t>(), status.as<uint8_t>()};
    }
};

void put16(uint8_t* p, uint32_t v) { p[0] = v >> 8, p[1] = v & 0xFF; }
void put32(uint8_t* p, uint32_t v) { put16(p, v >> 16), put16(p + 2, v & 0xFFFF); }

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
    std::mt19937 rng(78);

    const uint64_t n = uint64_t(sccsum_eth_tile_packets()) + 300;
    constexpr uint32_t kSlot = 96, kChannels = 70;
    const uint32_t host_ip = 0x0A000001u;
    std::vector<uint16_t> bound(kChannels);
    for (uint32_t k = 0; k < kChannels; ++k) bound[k] = static_cast<uint16_t>(2000 + 3 * k);
    const udp_ports ports(0, bound.data(), kChannels);
    if (ports.channels() != kChannels || ports.lookup(2003) != 1 || ports.lookup(2001) != -1) {
        std::printf("MISMATCH ports.lookup\n");
        ++bad;
    }

    // IPv4 packets to host_ip: mostly UDP to a bound port, some to an unbound one, some short, some TCP
    std::vector<uint8_t> bytes(n * kSlot + 16);
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> len(n), index(n), src_of(n);
    std::vector<uint8_t> status(n);
    for (auto& b : bytes) b = static_cast<uint8_t>(rng());
    for (uint64_t i = 0; i < n; ++i) {
        off[i] = i * kSlot + 8 + i % 16;
        const uint32_t kind = rng() % 10, ihl = 5 + rng() % 3;
        const uint32_t l4 = kind == 9 ? rng() % 8 : 8 + rng() % 30;
        len[i] = 4 * ihl + l4 + rng() % 3;  // some padded past the IP length
        uint8_t* h = &bytes[off[i]];
        h[0] = 0x40 | ihl;
        put16(h + 2, 4 * ihl + l4);
        put16(h + 6, 0);
        h[9] = kind == 8 ? 6 : 17;
        src_of[i] = 0x0A000100u + rng() % 50;
        put32(h + 12, src_of[i]);
        put32(h + 16, i % 23 == 5 ? host_ip + 1 : host_ip);
        put16(h + 4 * ihl + 2, kind < 7 ? bound[rng() % kChannels] : 2001);
        status[i] = rng() % 8 ? SCCSUM_ST_OK : static_cast<uint8_t>(rng() % 32);
        index[i] = static_cast<uint32_t>((i * 7) % n);  // a permutation: 7 does not divide n
    }
    index[3] = static_cast<uint32_t>(n);                 // out of range: skipped
    dev_array d_bytes(bytes.size()), d_off(8 * n), d_len(4 * n), d_status(n), d_index(4 * n);
    upload(d_bytes, bytes);
    upload(d_off, off);
    upload(d_len, len);
    upload(d_status, status);
    upload(d_index, index);

    // ---- udp_rx::run against sccsum_udp_rx
    const udp_rx rx(ports, host_ip);
    const device_packet_batch ip{d_bytes.p, bytes.size(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), n, 0};
    const uint32_t need = SCCSUM_ST_OK, reject = SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE | SCCSUM_ST_IPFRAG;
    rx_set ra(n, kChannels), rb(n, kChannels);
    rx.run(ip, d_status.as<uint8_t>(), d_index.as<uint32_t>(), n, ra.out(), ra.ws.p, stream);
    const udp_rx::outputs ob = rb.out();
    c_ok(sccsum_udp_rx(d_bytes.p, bytes.size(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), n, d_status.as<uint8_t>(),
                       need, reject, host_ip, ports.get(), d_index.as<uint32_t>(), n, ob.cls, ob.first, ob.order,
                       ob.pay_off, ob.pay_len, ob.src, ob.sport, rb.ws.p, stream),
         "sccsum_udp_rx");
    HIP_OK(hipStreamSynchronize(stream));
    ra.compare("rx", rb, true);
    std::vector<uint32_t> first(kChannels + 2);
    HIP_OK(hipMemcpy(first.data(), ra.first.p, 4 * first.size(), hipMemcpyDeviceToHost));
    const uint64_t delivered = first[kChannels], dropped = first[kChannels + 1] - first[kChannels];
    if (first[kChannels + 1] != n || delivered < n / 3 || dropped < n / 10 || first[1] == 0) {
        std::printf("MISMATCH rx.first values: %llu delivered, %llu dropped\n",
                    static_cast<unsigned long long>(delivered), static_cast<unsigned long long>(dropped));
        ++bad;
    }

    // ---- udp_rx::run_reassembled against sccsum_udp_rx_reasm: packet i's L4 part as a datagram of two
    // descriptors (3 bytes, the rest), its addresses in record (i + 1) % n
    std::vector<sccsum_gather_desc> desc;
    std::vector<uint32_t> dfirst(n + 1), dlen(n), dhead(n);
    std::vector<uint64_t> doff(n);
    std::vector<sccsum_frag_rec> rec(n);
    std::vector<uint8_t> l4_status(n);
    uint64_t at = 1000;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* h = &bytes[off[i]];
        const uint32_t hl = 4 * (h[0] & 0xF), e = ((uint32_t(h[2]) << 8) | h[3]) - hl;
        dfirst[i] = static_cast<uint32_t>(desc.size());
        doff[i] = at;
        dlen[i] = e;
        const uint32_t cut = e < 3 ? e : 3;
        if (cut) desc.push_back({d_bytes.p + off[i] + hl, static_cast<uint32_t>(at), cut});
        if (e > cut) desc.push_back({d_bytes.p + off[i] + hl + cut, static_cast<uint32_t>(at + cut), e - cut});
        at += e;
        dhead[i] = static_cast<uint32_t>((i + 1) % n);
        sccsum_frag_rec& r = rec[(i + 1) % n];
        std::memset(&r, 0, sizeof(r));
        r.src = src_of[i];
        r.dst = i % 23 == 5 ? host_ip + 1 : host_ip;
        r.proto = h[9];
        l4_status[i] = rng() % 6 ? SCCSUM_ST_OK : 0;
    }
    dfirst[n] = static_cast<uint32_t>(desc.size());
    dhead[7] = static_cast<uint32_t>(n);  // no such record: skipped
    dev_array d_desc(16 * desc.size()), d_dfirst(4 * (n + 1)), d_doff(8 * n), d_dlen(4 * n), d_dhead(4 * n),
        d_rec(sizeof(sccsum_frag_rec) * n), d_l4(n);
    upload(d_desc, desc);
    upload(d_dfirst, dfirst);
    upload(d_doff, doff);
    upload(d_dlen, dlen);
    upload(d_dhead, dhead);
    upload(d_rec, rec);
    upload(d_l4, l4_status);
    const udp_rx::datagrams in{d_desc.as<sccsum_gather_desc>(), d_dfirst.as<uint32_t>(), d_doff.as<uint64_t>(),
                               d_dlen.as<uint32_t>(),           d_dhead.as<uint32_t>(),  n,
                               d_rec.as<sccsum_frag_rec>(),     n};
    rx_set ma(n, kChannels), mb(n, kChannels);
    rx.run_reassembled(in, d_l4.as<uint8_t>(), ma.out(), ma.ws.p, stream, SCCSUM_ST_OK, SCCSUM_ST_RANGE);
    const udp_rx::outputs om = mb.out();
    c_ok(sccsum_udp_rx_reasm(in.desc, in.dgram_first, in.dgram_off, in.dgram_len, in.dgram_head, n, in.rec, n,
                             d_l4.as<uint8_t>(), SCCSUM_ST_OK, SCCSUM_ST_RANGE, host_ip, ports.get(), om.cls, om.first,
                             om.order, om.pay_len, om.src, om.sport, mb.ws.p, stream),
         "sccsum_udp_rx_reasm");
    HIP_OK(hipStreamSynchronize(stream));
    ma.compare("reasm", mb, false);
    same("reasm.pay_off (not written)", ma.pay_off, mb.pay_off);
    HIP_OK(hipMemcpy(first.data(), ma.first.p, 4 * first.size(), hipMemcpyDeviceToHost));
    if (first[kChannels + 1] != n || first[kChannels] < n / 3 || first[kChannels] == n) {
        std::printf("MISMATCH reasm.first values\n");
        ++bad;
    }

    // ---- udp_tx::run against sccsum_udp_send: the packets' payloads behind their 8 bytes of headroom, on
    // two copies of the buffer; some too close to the buffer's start or past its end
    std::vector<uint64_t> poff(n);
    std::vector<uint32_t> plen(n), dst(n);
    std::vector<uint16_t> dport(n), sport(n);
    for (uint64_t i = 0; i < n; ++i) {
        poff[i] = i * kSlot + 8 + i % 16;
        plen[i] = rng() % 70;
        dst[i] = 0x0A000100u + rng() % 50;
        dport[i] = static_cast<uint16_t>(rng());
        sport[i] = static_cast<uint16_t>(rng());
    }
    poff[0] = 7;
    poff[5] = bytes.size() - 3;
    plen[5] = 4;
    plen[9] = 65508;
    dev_array d_poff(8 * n), d_plen(4 * n), d_dst(4 * n), d_dport(2 * n), d_sport(2 * n);
    upload(d_poff, poff);
    upload(d_plen, plen);
    upload(d_dst, dst);
    upload(d_dport, dport);
    upload(d_sport, sport);
    const sccsum_udp_opts opts = {host_ip, 68, SCCSUM_UDP_CSUM_OFFLOAD};
    const udp_tx tx(opts);
    tx_set ta(bytes.size(), n), tb(bytes.size(), n);
    upload(ta.bytes, bytes);
    upload(tb.bytes, bytes);
    tx.run(ta.bytes.p, bytes.size(), d_poff.as<uint64_t>(), d_plen.as<uint32_t>(), n, d_dst.as<uint32_t>(),
           d_dport.as<uint16_t>(), d_sport.as<uint16_t>(), ta.out(), stream);
    const udp_tx::outputs ot = tb.out();
    c_ok(sccsum_udp_send(&opts, tb.bytes.p, bytes.size(), d_poff.as<uint64_t>(), d_plen.as<uint32_t>(),
                         d_dst.as<uint32_t>(), d_dport.as<uint16_t>(), d_sport.as<uint16_t>(), n, ot.l4_off, ot.l4_len,
                         ot.sum_len, ot.seed, ot.proto, ot.needs_csum, ot.status, stream),
         "sccsum_udp_send");
    HIP_OK(hipStreamSynchronize(stream));
    same("tx.bytes", ta.bytes, tb.bytes);
    same("tx.l4_off", ta.l4_off, tb.l4_off);
    same("tx.l4_len", ta.l4_len, tb.l4_len);
    same("tx.sum_len", ta.sum_len, tb.sum_len);
    same("tx.seed", ta.seed, tb.seed);
    same("tx.proto", ta.proto, tb.proto);
    same("tx.needs_csum", ta.needs_csum, tb.needs_csum);
    same("tx.status", ta.status, tb.status);
    const std::vector<uint8_t> st = ta.status.host(), nc = ta.needs_csum.host(), sent = ta.bytes.host();
    uint64_t ok = 0, offloaded = 0;
    for (uint64_t i = 0; i < n; ++i) {
        ok += st[i] == SCCSUM_ST_OK;
        offloaded += nc[i];
    }
    if (st[0] != SCCSUM_ST_RANGE || st[5] != SCCSUM_ST_RANGE || !(st[9] & SCCSUM_ST_MALFORMED) || ok != n - 3 ||
        offloaded == 0 || offloaded == ok || std::memcmp(sent.data(), bytes.data(), bytes.size()) == 0) {
        std::printf("MISMATCH tx.status values\n");
        ++bad;
    }

    HIP_OK(hipStreamDestroy(stream));
    if (bad) return 1;
    std::printf("udp_gpu: OK (%llu packets, %llu with a channel, %llu of %llu datagrams sent, %llu offloaded)\n",
                static_cast<unsigned long long>(n), static_cast<unsigned long long>(delivered),
                static_cast<unsigned long long>(ok), static_cast<unsigned long long>(n),
                static_cast<unsigned long long>(offloaded));
    return 0;
}
