// Native host program over the C++ classes arp_table, eth_rx and eth_tx
// (seastar/net/ip_checksum_batch.hh): each forwards a dozen or more arguments,
// many of one type, to a C call that the Python tests pin.  Here the wrapper
// and the C call it forwards to run on the same inputs into two separately
// poisoned sets of outputs (64 guard bytes behind each array, the workspaces
// poisoned too), every optional argument given, and every array must be
// byte-equal: a swapped or dropped argument shows.  The inputs span a tile
// edge: a tile + 300 wire frames (IPv4, ARP, unknown, short), their IPv4
// bucket through the learn records, and the same frames' L3 parts as
// one-descriptor lists through eth_tx with a cap that cuts the batch.
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

void same_bytes(const char* name, const dev_array& a, const dev_array& b, const std::vector<uint8_t>& ha,
                const std::vector<uint8_t>& hb) {
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

// Both arrays byte for byte, guards included (both were poisoned alike), and the guards themselves.
void same(const char* name, const dev_array& a, const dev_array& b) { same_bytes(name, a, b, a.host(), b.host()); }

void c_ok(int rc, const char* what) {
    if (rc != SCCSUM_OK) {
        std::printf("%s: %s\n", what, sccsum_strerror(rc));
        std::exit(2);
    }
}

struct rx_set {
    dev_array cls, first, order, l3_off, l3_len, src_mac, ws;
    rx_set(uint64_t n, uint32_t k)
        : cls(n), first(4 * (k + 2)), order(4 * n), l3_off(8 * n), l3_len(4 * n), src_mac(8 * n),
          ws(eth_rx::workspace(n), 0x5A) {}
};

struct learn_set {
    dev_array rec, count, ws;
    explicit learn_set(uint64_t n) : rec(16 * n), count(4), ws(eth_rx::learn_workspace(n), 0x5A) {}
};

struct tx_set {
    dev_array eth, desc, first, out_off, out_len, frame_src, status, unresolved, total, ws;
    tx_set(uint64_t n, uint64_t frames, uint64_t descs)
        : eth(14 * frames), desc(16 * (descs + frames)), first(4 * (frames + 1)), out_off(8 * frames),
          out_len(4 * frames), frame_src(4 * frames), status(n), unresolved(8 * n), total(48),
          ws(eth_tx::workspace(n), 0x5A) {}
    eth_tx::outputs out() const {
        return eth_tx::outputs{eth.as<uint8_t>(),       desc.as<sccsum_gather_desc>(), first.as<uint32_t>(),
                               out_off.as<uint64_t>(),  out_len.as<uint32_t>(),        frame_src.as<uint32_t>(),
                               status.as<uint8_t>(),    unresolved.as<sccsum_eth_unresolved>(), total.as<uint64_t>()};
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
    std::mt19937 rng(77);

    const uint64_t n = uint64_t(sccsum_eth_tile_packets()) + 300;
    constexpr uint32_t kSlot = 96;
    const uint32_t host_ip = 0x0A000001u, netmask = 0xFFFF0000u, gw = 0x0A0000FEu;
    const uint64_t hw = 0x02AB12CD34EFull;

    // wire frames: mostly IPv4 from 10.0.x.y, some ARP, some unknown, some short
    std::vector<uint8_t> bytes(n * kSlot);
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> len(n);
    for (auto& b : bytes) b = static_cast<uint8_t>(rng());
    for (uint64_t i = 0; i < n; ++i) {
        off[i] = i * kSlot + i % 16;
        len[i] = 34 + rng() % 40;
        uint8_t* f = &bytes[off[i]];
        const uint32_t kind = rng() % 10;
        const uint16_t proto = kind < 7 ? 0x0800 : kind == 7 ? 0x0806 : 0x86DD;
        f[12] = proto >> 8;
        f[13] = proto & 0xFF;
        if (kind == 9) len[i] = rng() % 14;
        const uint32_t src = rng() % 4 ? 0x0A000000u + rng() % 64 : 0x0B000000u + rng() % 64;
        f[26] = src >> 24, f[27] = (src >> 16) & 0xFF, f[28] = (src >> 8) & 0xFF, f[29] = src & 0xFF;
    }
    dev_array d_bytes(bytes.size()), d_off(8 * n), d_len(4 * n);
    upload(d_bytes, bytes);
    upload(d_off, off);
    upload(d_len, len);

    // ---- eth_rx::run against sccsum_eth_rx
    const eth_rx rx({0x0800, 0x0806});
    const uint16_t protos[2] = {0x0800, 0x0806};
    const device_packet_batch wire{d_bytes.p, bytes.size(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), n, 0};
    rx_set ra(n, 2), rb(n, 2);
    rx.run(wire, eth_rx::outputs{ra.cls.as<uint8_t>(), ra.first.as<uint32_t>(), ra.order.as<uint32_t>(),
                                 ra.l3_off.as<uint64_t>(), ra.l3_len.as<uint32_t>(), ra.src_mac.as<uint64_t>()},
           ra.ws.p, stream);
    c_ok(sccsum_eth_rx(d_bytes.p, bytes.size(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), n, protos, 2,
                       rb.cls.as<uint8_t>(), rb.first.as<uint32_t>(), rb.order.as<uint32_t>(), rb.l3_off.as<uint64_t>(),
                       rb.l3_len.as<uint32_t>(), rb.src_mac.as<uint64_t>(), rb.ws.p, stream),
         "sccsum_eth_rx");
    HIP_OK(hipStreamSynchronize(stream));
    same("rx.cls", ra.cls, rb.cls);
    same("rx.first", ra.first, rb.first);
    same("rx.order", ra.order, rb.order);
    same("rx.l3_off", ra.l3_off, rb.l3_off);
    same("rx.l3_len", ra.l3_len, rb.l3_len);
    same("rx.src_mac", ra.src_mac, rb.src_mac);
    uint32_t first[4];
    HIP_OK(hipMemcpy(first, ra.first.p, sizeof(first), hipMemcpyDeviceToHost));
    const uint64_t n_ip = first[1] - first[0];
    if (first[3] != n || n_ip < n / 2 || first[2] == first[1] || first[3] == first[2]) {
        std::printf("MISMATCH rx.first values %u %u %u %u\n", first[0], first[1], first[2], first[3]);
        ++bad;
    }

    // ---- the table: half of the subnet's peers known with the MAC they send from
    std::vector<uint64_t> macs(n);
    HIP_OK(hipMemcpy(macs.data(), ra.src_mac.p, 8 * n, hipMemcpyDeviceToHost));
    std::vector<uint64_t> l3_off(n);
    HIP_OK(hipMemcpy(l3_off.data(), ra.l3_off.p, 8 * n, hipMemcpyDeviceToHost));
    std::vector<sccsum_arp_entry> entries = {{0xFFFFFFFFu, 0, 0xFFFFFFFFFFFFull}, {gw, 0, 0x02000000FFFEull}};
    for (uint64_t j = 0; j < n_ip; j += 2) {
        const uint8_t* h = &bytes[l3_off[j]];
        entries.push_back({uint32_t(h[12]) << 24 | uint32_t(h[13]) << 16 | uint32_t(h[14]) << 8 | h[15], 0, macs[j]});
    }
    const arp_table arp(0, entries.data(), static_cast<uint32_t>(entries.size()));
    uint64_t mac = 0;
    if (!arp.lookup(gw, &mac) || mac != 0x02000000FFFEull || arp.lookup(0x01020304u, &mac)) {
        std::printf("MISMATCH arp.lookup\n");
        ++bad;
    }

    // ---- eth_rx::learn against sccsum_arp_learn_records, on the IPv4 bucket
    dev_array d_status(n_ip);
    std::vector<uint8_t> status(n_ip);
    for (auto& s : status) s = rng() % 8 ? SCCSUM_ST_OK : static_cast<uint8_t>(rng() % 32);
    upload(d_status, status);
    const device_packet_batch ip{d_bytes.p, bytes.size(), ra.l3_off.as<uint64_t>(), ra.l3_len.as<uint32_t>(), n_ip, 0};
    learn_set la(n_ip), lb(n_ip);
    eth_rx::learn(ip, d_status.as<uint8_t>(), ra.src_mac.as<uint64_t>(), host_ip, netmask, &arp,
                  la.rec.as<sccsum_arp_rec>(), la.count.as<uint32_t>(), la.ws.p, stream);
    c_ok(sccsum_arp_learn_records(d_bytes.p, bytes.size(), ra.l3_off.as<uint64_t>(), ra.l3_len.as<uint32_t>(),
                                  d_status.as<uint8_t>(), SCCSUM_ST_OK, SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE,
                                  ra.src_mac.as<uint64_t>(), n_ip, host_ip, netmask, arp.get(),
                                  lb.rec.as<sccsum_arp_rec>(), lb.count.as<uint32_t>(), lb.ws.p, stream),
         "sccsum_arp_learn_records");
    HIP_OK(hipStreamSynchronize(stream));
    same("learn.rec", la.rec, lb.rec);
    same("learn.count", la.count, lb.count);
    uint32_t count = 0;
    HIP_OK(hipMemcpy(&count, la.count.p, 4, hipMemcpyDeviceToHost));
    if (count == 0 || count >= n_ip) {
        std::printf("MISMATCH learn.count value %u of %llu\n", count, static_cast<unsigned long long>(n_ip));
        ++bad;
    }

    // ---- eth_tx::run against sccsum_eth_send: the bucket's L3 parts as one-descriptor frames, one per
    // datagram, sent back to their sources (known, unknown, and off the subnet: the gateway)
    std::vector<uint32_t> l3_len(n);
    HIP_OK(hipMemcpy(l3_len.data(), ra.l3_len.p, 4 * n, hipMemcpyDeviceToHost));
    std::vector<sccsum_gather_desc> desc(n_ip);
    std::vector<uint32_t> dfirst(n_ip + 1), dst(n_ip), flen(n_ip);
    std::vector<uint64_t> foff(n_ip);
    uint64_t at = 4096, need_bytes = 0;
    for (uint64_t j = 0; j < n_ip; ++j) {
        const uint8_t* h = &bytes[l3_off[j]];
        dst[j] = uint32_t(h[12]) << 24 | uint32_t(h[13]) << 16 | uint32_t(h[14]) << 8 | h[15];
        if (j % 11 == 3) dst[j] = 0x0A00FF00u + j % 7;  // on the subnet, never seen: unresolved
        desc[j] = {d_bytes.p + l3_off[j], static_cast<uint32_t>(at), l3_len[j]};
        dfirst[j] = static_cast<uint32_t>(j);
        foff[j] = at;
        flen[j] = l3_len[j];
        at += l3_len[j];
        need_bytes += l3_len[j] + 14;
    }
    dfirst[n_ip] = static_cast<uint32_t>(n_ip);
    dev_array d_desc(16 * n_ip), d_first(4 * (n_ip + 1)), d_dgram_first(4 * (n_ip + 1)), d_dst(4 * n_ip), d_foff(8 * n_ip),
        d_flen(4 * n_ip);
    upload(d_desc, desc);
    upload(d_first, dfirst);
    upload(d_dgram_first, dfirst);
    upload(d_dst, dst);
    upload(d_foff, foff);
    upload(d_flen, flen);
    const sccsum_eth_opts opts = {hw, host_ip, netmask, gw, 0x0800};
    const eth_tx tx(opts);
    const uint64_t cap = need_bytes / 2;  // cuts the batch: the prefix rule runs
    tx_set ta(n_ip, n_ip, n_ip), tb(n_ip, n_ip, n_ip);
    tx.run(arp, d_dst.as<uint32_t>(), d_dgram_first.as<uint32_t>(), n_ip, d_desc.as<sccsum_gather_desc>(),
           d_first.as<uint32_t>(), d_foff.as<uint64_t>(), d_flen.as<uint32_t>(), n_ip, cap, ta.out(), ta.ws.p, stream);
    const eth_tx::outputs ob = tb.out();
    c_ok(sccsum_eth_send(&opts, arp.get(), d_dst.as<uint32_t>(), d_dgram_first.as<uint32_t>(), n_ip,
                         d_desc.as<sccsum_gather_desc>(), d_first.as<uint32_t>(), d_foff.as<uint64_t>(),
                         d_flen.as<uint32_t>(), n_ip, cap, ob.eth, ob.desc, ob.first, ob.out_off, ob.out_len,
                         ob.frame_src, ob.status, ob.unresolved, ob.total, tb.ws.p, stream),
         "sccsum_eth_send");
    HIP_OK(hipStreamSynchronize(stream));
    same("tx.eth", ta.eth, tb.eth);
    same("tx.first", ta.first, tb.first);
    same("tx.out_off", ta.out_off, tb.out_off);
    same("tx.out_len", ta.out_len, tb.out_len);
    same("tx.frame_src", ta.frame_src, tb.frame_src);
    same("tx.status", ta.status, tb.status);
    same("tx.unresolved", ta.unresolved, tb.unresolved);
    same("tx.total", ta.total, tb.total);
    uint64_t total[6];
    HIP_OK(hipMemcpy(total, ta.total.p, sizeof(total), hipMemcpyDeviceToHost));
    if (total[2] == 0 || total[2] >= n_ip || total[3] == 0 || total[4] == 0 || total[5] != 2 * total[4] ||
        total[1] <= cap) {
        std::printf("MISMATCH tx.total values\n");
        ++bad;
    }
    // the Ethernet descriptors hold their own set's d_eth address: take it out before comparing
    std::vector<uint8_t> ha = ta.desc.host(), hb = tb.desc.host();
    for (uint64_t f = 0; f < total[4]; ++f) {
        for (auto* hv : {&ha, &hb}) {
            uint64_t src;
            std::memcpy(&src, hv->data() + 32 * f, 8);
            src -= reinterpret_cast<uint64_t>(hv == &ha ? ta.eth.p : tb.eth.p);
            std::memcpy(hv->data() + 32 * f, &src, 8);
        }
    }
    same_bytes("tx.desc", ta.desc, tb.desc, ha, hb);

    HIP_OK(hipStreamDestroy(stream));
    if (bad) return 1;
    std::printf("eth_gpu: OK (%llu frames, %llu IPv4, %u learn records, %llu of %llu datagrams sent)\n",
                static_cast<unsigned long long>(n), static_cast<unsigned long long>(n_ip), count,
                static_cast<unsigned long long>(total[4]), static_cast<unsigned long long>(n_ip));
    return 0;
}
