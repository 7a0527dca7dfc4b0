// Native host program over the C++ classes tcp_conns, tcp_rx and tcp_tx
// (seastar/net/ip_checksum_batch.hh): tcp_rx::run forwards 25 arguments and
// tcp_tx::run 16, many of one type, to C calls that the Python tests pin.
// Here the wrapper and the C call it forwards to run on the same inputs into
// two separately poisoned sets of outputs (64 guard bytes behind each array,
// the workspaces poisoned too), every optional argument given, and every array
// must be byte-equal: a swapped or dropped argument, or a field of an outputs
// struct mapped to the wrong parameter, shows.  The inputs span a tile edge: a
// tile + 300 IPv4 packets (TCP to known connections, to listening and to
// closed ports with and without RST, short ones, UDP, another host's) through
// tcp_rx::run with an index, non-default masks and the offload form of the
// answers, and their payloads through tcp_tx::run on two copies of the buffer.
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
    dev_array cls, first, order, seg, src, run_conn, run_first, rst, rst_dst, total, ws;
    rx_set(uint64_t n, uint64_t runs, uint64_t ws_bytes)
        : cls(n), first(4 * 5), order(4 * n), seg(sizeof(sccsum_tcp_seg) * n), src(4 * n), run_conn(4 * runs),
          run_first(4 * runs), rst(20 * n), rst_dst(4 * n), total(8 * 4), ws(ws_bytes, 0x5A) {}
    tcp_rx::outputs out() const {
        tcp_rx::outputs o;
        o.cls = cls.as<uint8_t>();
        o.first = first.as<uint32_t>();
        o.order = order.as<uint32_t>();
        o.seg = seg.as<sccsum_tcp_seg>();
        o.src = src.as<uint32_t>();
        o.run_conn = run_conn.as<uint32_t>();
        o.run_first = run_first.as<uint32_t>();
        o.rst = rst.p;
        o.rst_dst = rst_dst.as<uint32_t>();
        o.total = total.as<uint64_t>();
        return o;
    }
    void compare(const rx_set& o) const {
        same("rx.cls", cls, o.cls);
        same("rx.first", first, o.first);
        same("rx.order", order, o.order);
        same("rx.seg", seg, o.seg);
        same("rx.src", src, o.src);
        same("rx.run_conn", run_conn, o.run_conn);
        same("rx.run_first", run_first, o.run_first);
        same("rx.rst", rst, o.rst);
        same("rx.rst_dst", rst_dst, o.rst_dst);
        same("rx.total", total, o.total);
    }
};

struct tx_set {
    dev_array bytes, l4_off, l4_len, sum_len, seed, tso_seg, proto, needs_csum, status;
    tx_set(size_t nbytes, uint64_t n)
        : bytes(nbytes), l4_off(8 * n), l4_len(4 * n), sum_len(4 * n), seed(4 * n), tso_seg(2 * n), proto(n),
          needs_csum(n), status(n) {}
    tcp_tx::outputs out() const {
        tcp_tx::outputs o;
        o.l4_off = l4_off.as<uint64_t>();
        o.l4_len = l4_len.as<uint32_t>();
        o.sum_len = sum_len.as<uint32_t>();
        o.seed = seed.as<uint32_t>();
        o.tso_seg = tso_seg.as<uint16_t>();
        o.proto = proto.as<uint8_t>();
        o.needs_csum = needs_csum.as<uint8_t>();
        o.status = status.as<uint8_t>();
        return o;
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
    std::mt19937 rng(79);

    const uint64_t n = uint64_t(sccsum_eth_tile_packets()) + 300;
    constexpr uint32_t kSlot = 128, kConns = 300;   // 300 connections: two passes of the sort
    const uint32_t host_ip = 0x0A000001u;
    std::vector<sccsum_tcp_conn> ids(kConns);
    for (uint32_t c = 0; c < kConns; ++c) {
        ids[c] = {host_ip, 0x0A000100u + c / 2, static_cast<uint16_t>(80 + c % 2), static_cast<uint16_t>(30000 + c)};
    }
    const uint16_t listening[2] = {22, 8080};
    const tcp_conns conns(0, ids.data(), kConns, listening, 2);
    if (conns.count() != kConns || conns.bits() != 10 || conns.lookup(ids[7]) != 7 || !conns.listening(22) ||
        conns.listening(80) || conns.lookup({host_ip, 0x0A000100u, 80, 29999}) != -1) {
        std::printf("MISMATCH conns\n");
        ++bad;
    }

    // IPv4 packets: mostly TCP of a known connection, some to a listening and some to a closed port, short
    // ones, a header longer than the segment, UDP, another host's
    std::vector<uint8_t> bytes(n * kSlot + 16);
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> len(n), index(n);
    std::vector<uint8_t> status(n);
    for (auto& b : bytes) b = static_cast<uint8_t>(rng());
    for (uint64_t i = 0; i < n; ++i) {
        off[i] = i * kSlot + 8 + i % 16;
        const uint32_t kind = rng() % 12, ihl = 5 + rng() % 3, doff = kind == 10 ? 4 + rng() % 11 : 5 + rng() % 2;
        const uint32_t l4 = kind == 11 ? rng() % 20 : kind == 10 ? 20 + rng() % 8 : 4 * doff + rng() % 30;
        len[i] = 4 * ihl + l4 + rng() % 3;  // some padded past the IP length
        uint8_t* h = &bytes[off[i]];
        h[0] = 0x40 | ihl;
        put16(h + 2, 4 * ihl + l4);
        put16(h + 6, 0);
        h[9] = kind == 9 ? 17 : 6;
        const sccsum_tcp_conn& id = ids[rng() % kConns];
        put32(h + 12, kind == 6 ? id.foreign_ip + 0x1000 : id.foreign_ip);
        put32(h + 16, i % 23 == 5 ? host_ip + 1 : host_ip);
        uint8_t* t = h + 4 * ihl;
        put16(t, id.foreign_port);
        put16(t + 2, kind == 7 ? 22 : kind == 8 ? 443 : id.local_port);
        t[12] = static_cast<uint8_t>((doff << 4) | (t[12] & 0xF));
        if (kind == 8 && rng() % 4) t[13] &= ~0x04;  // mostly answered, some RSTs discarded
        status[i] = rng() % 8 ? (SCCSUM_ST_OK | SCCSUM_ST_L4_OK) : static_cast<uint8_t>(rng() % 32);
        index[i] = static_cast<uint32_t>((i * 7) % n);  // a permutation: 7 does not divide n
    }
    index[3] = static_cast<uint32_t>(n);                 // out of range: skipped
    dev_array d_bytes(bytes.size()), d_off(8 * n), d_len(4 * n), d_status(n), d_index(4 * n);
    upload(d_bytes, bytes);
    upload(d_off, off);
    upload(d_len, len);
    upload(d_status, status);
    upload(d_index, index);

    // ---- tcp_rx::run against sccsum_tcp_rx
    const tcp_rx rx(conns, host_ip, SCCSUM_TCP_CSUM_OFFLOAD);
    const device_packet_batch ip{d_bytes.p, bytes.size(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), n, 0};
    const uint32_t need = SCCSUM_ST_OK, reject = SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE;   // not the defaults
    if (rx.workspace(n) != sccsum_tcp_rx_workspace(n, kConns)) {
        std::printf("MISMATCH rx.workspace\n");
        ++bad;
    }
    rx_set ra(n, kConns + 1, rx.workspace(n)), rb(n, kConns + 1, rx.workspace(n));
    rx.run(ip, d_status.as<uint8_t>(), d_index.as<uint32_t>(), n, ra.out(), ra.ws.p, stream, need, reject);
    const tcp_rx::outputs ob = rb.out();
    c_ok(sccsum_tcp_rx(d_bytes.p, bytes.size(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), n, d_status.as<uint8_t>(),
                       need, reject, host_ip, conns.get(), d_index.as<uint32_t>(), n, SCCSUM_TCP_CSUM_OFFLOAD, ob.cls,
                       ob.first, ob.order, ob.seg, ob.src, ob.run_conn, ob.run_first, ob.rst, ob.rst_dst, ob.total,
                       rb.ws.p, stream),
         "sccsum_tcp_rx");
    HIP_OK(hipStreamSynchronize(stream));
    ra.compare(rb);
    uint32_t first[5];
    uint64_t total[4];
    HIP_OK(hipMemcpy(first, ra.first.p, sizeof(first), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(total, ra.total.p, sizeof(total), hipMemcpyDeviceToHost));
    const uint64_t known = first[1], listen = first[2] - first[1], resets = first[3] - first[2];
    if (first[0] != 0 || first[4] != n || known < n / 4 || listen < n / 40 || resets < n / 40 || total[1] != resets ||
        total[0] < kConns / 2 || total[0] > kConns || first[4] - first[3] < n / 10) {
        std::printf("MISMATCH rx.first values: %llu known, %llu listen, %llu resets, %llu runs\n",
                    static_cast<unsigned long long>(known), static_cast<unsigned long long>(listen),
                    static_cast<unsigned long long>(resets), static_cast<unsigned long long>(total[0]));
        ++bad;
    }
    // the answers carry the offload form: the folded pseudo-header sum of {local, foreign, 6, 20}
    {
        const std::vector<uint8_t> rst = ra.rst.host(), dst = ra.rst_dst.host(), order = ra.order.host();
        for (uint64_t r = 0; r < resets; ++r) {
            uint32_t foreign, idx;
            std::memcpy(&foreign, &dst[4 * r], 4);
            std::memcpy(&idx, &order[4 * (first[2] + r)], 4);
            const uint8_t* h = &bytes[off[idx]];
            const uint32_t local = (uint32_t(h[16]) << 24) | (uint32_t(h[17]) << 16) | (uint32_t(h[18]) << 8) | h[19];
            const uint32_t want = sccsum_pseudo_seed(local, foreign, 6, 20);
            if (((uint32_t(rst[20 * r + 16]) << 8) | rst[20 * r + 17]) != want || !(rst[20 * r + 13] & 0x04)) {
                std::printf("MISMATCH rx.rst %llu: not the offload form\n", static_cast<unsigned long long>(r));
                ++bad;
                break;
            }
        }
    }

    // ---- tcp_tx::run against sccsum_tcp_send: payloads behind their headroom, on two copies of the
    // buffer; some too close to the buffer's start or past its end, bad header lengths, no mss
    std::vector<uint64_t> poff(n);
    std::vector<uint32_t> plen(n);
    std::vector<sccsum_tcp_out> out(n);
    for (uint64_t i = 0; i < n; ++i) {
        out[i].hdr_len = static_cast<uint8_t>(20 + 4 * (rng() % 6));   // at most 40: inside the slot
        poff[i] = i * kSlot + 44 + i % 16;
        plen[i] = rng() % 60;
        out[i].dst = 0x0A000100u + rng() % 50;
        out[i].seq = static_cast<uint32_t>(rng());
        out[i].ack = static_cast<uint32_t>(rng());
        out[i].sport = static_cast<uint16_t>(rng());
        out[i].dport = static_cast<uint16_t>(rng());
        out[i].window = static_cast<uint16_t>(rng());
        out[i].flags = static_cast<uint8_t>(rng());
        out[i].mss = 1 + rng() % 60;                                   // below and above the length
    }
    poff[0] = 19;
    poff[5] = bytes.size() - 3;
    plen[5] = 4;
    plen[9] = 65515;
    out[11].hdr_len = 22;
    out[12].hdr_len = 64;
    out[13].mss = 0;
    dev_array d_poff(8 * n), d_plen(4 * n), d_out(sizeof(sccsum_tcp_out) * n);
    upload(d_poff, poff);
    upload(d_plen, plen);
    upload(d_out, out);
    const sccsum_tcp_opts opts = {host_ip, 1500, SCCSUM_TCP_CSUM_OFFLOAD | SCCSUM_TCP_TSO};
    const tcp_tx tx(opts);
    tx_set ta(bytes.size(), n), tb(bytes.size(), n);
    upload(ta.bytes, bytes);
    upload(tb.bytes, bytes);
    tx.run(ta.bytes.p, bytes.size(), d_poff.as<uint64_t>(), d_plen.as<uint32_t>(), d_out.as<sccsum_tcp_out>(), n,
           ta.out(), stream);
    const tcp_tx::outputs ot = tb.out();
    c_ok(sccsum_tcp_send(&opts, tb.bytes.p, bytes.size(), d_poff.as<uint64_t>(), d_plen.as<uint32_t>(),
                         d_out.as<sccsum_tcp_out>(), n, ot.l4_off, ot.l4_len, ot.sum_len, ot.seed, ot.tso_seg, ot.proto,
                         ot.needs_csum, ot.status, stream),
         "sccsum_tcp_send");
    HIP_OK(hipStreamSynchronize(stream));
    same("tx.bytes", ta.bytes, tb.bytes);
    same("tx.l4_off", ta.l4_off, tb.l4_off);
    same("tx.l4_len", ta.l4_len, tb.l4_len);
    same("tx.sum_len", ta.sum_len, tb.sum_len);
    same("tx.seed", ta.seed, tb.seed);
    same("tx.tso_seg", ta.tso_seg, tb.tso_seg);
    same("tx.proto", ta.proto, tb.proto);
    same("tx.needs_csum", ta.needs_csum, tb.needs_csum);
    same("tx.status", ta.status, tb.status);
    const std::vector<uint8_t> st = ta.status.host(), nc = ta.needs_csum.host(), sent = ta.bytes.host(),
                               tso = ta.tso_seg.host();
    uint64_t ok = 0, offloaded = 0, big = 0;
    for (uint64_t i = 0; i < n; ++i) {
        ok += st[i] == SCCSUM_ST_OK;
        offloaded += nc[i];
        big += (tso[2 * i] | tso[2 * i + 1]) != 0;
    }
    if (st[0] != SCCSUM_ST_RANGE || st[5] != SCCSUM_ST_RANGE || !(st[9] & SCCSUM_ST_MALFORMED) ||
        st[11] != SCCSUM_ST_MALFORMED || st[12] != SCCSUM_ST_MALFORMED || st[13] != SCCSUM_ST_MALFORMED || ok != n - 6 ||
        offloaded != ok || big == 0 || big == ok || std::memcmp(sent.data(), bytes.data(), bytes.size()) == 0) {
        std::printf("MISMATCH tx.status values\n");
        ++bad;
    }

    HIP_OK(hipStreamDestroy(stream));
    if (bad) return 1;
    std::printf("tcp_gpu: OK (%llu packets: %llu of known connections in %llu runs, %llu for listeners, %llu answered; "
                "%llu of %llu segments sent, %llu with a TSO size)\n",
                static_cast<unsigned long long>(n), static_cast<unsigned long long>(known),
                static_cast<unsigned long long>(total[0]), static_cast<unsigned long long>(listen),
                static_cast<unsigned long long>(resets), static_cast<unsigned long long>(ok),
                static_cast<unsigned long long>(n), static_cast<unsigned long long>(big));
    return 0;
}
