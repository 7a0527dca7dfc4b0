// Host-only program over the TCP-layer C calls and their C++ classes
// (seastar/net/ip_checksum_batch.hh: tcp_conns, tcp_rx, tcp_tx): the
// connection table's lookup against a std::map (every entry, misses differing
// in one field, colliding keys built with slot(), a probe run that wraps, all
// 65 536 ports), duplicates refused, the classes' workspace() and taken()
// against the C calls, and argument errors of the two device calls through
// the classes, which the library reports before any device work.  No launch
// is made: it runs without a device.  tests/test_tcp_host.py builds it against
// the library and, with tcp.hip compiled in, under ASan + UBSan.
// Prints "tcp_host: OK (...)" and exits 0; a failure names itself, exit 1.
#include <seastar/net/ip_checksum_batch.hh>

#include <array>
#include <cstdio>
#include <map>
#include <random>
#include <vector>

using namespace seastar::net;

namespace {

int bad = 0;

void expect(bool ok, const char* what, int line) {
    if (!ok) {
        std::printf("FAILED %s (line %d)\n", what, line);
        ++bad;
    }
}
#define EXPECT(x) expect((x), #x, __LINE__)

using key = std::array<uint32_t, 4>;

sccsum_tcp_conn conn_of(const key& k) {
    return {k[0], k[1], static_cast<uint16_t>(k[2]), static_cast<uint16_t>(k[3])};
}

size_t tables(std::mt19937& rng) {
    size_t entries = 0;
    for (uint32_t n : {0u, 1u, 8u, 9u, 253u, 4097u, 70000u}) {
        std::map<key, int64_t> want;
        std::vector<sccsum_tcp_conn> conns;
        const auto r = [&rng](uint32_t below) { return static_cast<uint32_t>(rng() % below); };
        while (conns.size() < n) {
            // few distinct values a field: many keys differ in one field only
            const key k = conns.empty() ? key{0, 0, 0, 0}
                          : conns.size() == 1 ? key{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFu, 0xFFFFu}
                                              : key{0x0A000001u + r(2), 0x0B000000u + r(n / 2 + 1), 80u + r(3),
                                                    1024u + r(16)};
            if (want.count(k)) continue;
            want[k] = static_cast<int64_t>(conns.size());
            conns.push_back(conn_of(k));
        }
        std::vector<uint16_t> listen;
        for (uint32_t q = 0; q < 65536 && listen.size() < n; q += 1 + n % 7) listen.push_back(static_cast<uint16_t>(q));
        const tcp_conns t(conns.data(), n, listen.data(), static_cast<uint32_t>(listen.size()));
        uint32_t bits = 4;
        while ((uint64_t(1) << bits) < 2ull * n) ++bits;
        EXPECT(t.count() == n && t.bits() == bits);
        for (const auto& [k, c] : want) {
            EXPECT(t.lookup(conn_of(k)) == c);
            for (int f = 0; f < 4; ++f) {
                key m = k;
                m[f] = f < 2 ? m[f] ^ 1u : (m[f] ^ 1u) & 0xFFFFu;
                const auto it = want.find(m);
                EXPECT(t.lookup(conn_of(m)) == (it == want.end() ? -1 : it->second));
            }
        }
        std::vector<bool> is(65536, false);
        for (uint16_t q : listen) is[q] = true;
        for (uint32_t q = 0; q < 65536; ++q) EXPECT(t.listening(static_cast<uint16_t>(q)) == is[q]);
        entries += n;
    }
    // six keys homed at the last of 16 slots: the run wraps; others of that home miss
    std::vector<sccsum_tcp_conn> run, others;
    for (uint32_t b = 1; others.size() < 4; ++b) {
        const sccsum_tcp_conn c{0x0A000001u, b, 80, 5000};
        if (tcp_conns::slot(c, 4) != 15) continue;
        (run.size() < 6 ? run : others).push_back(c);
    }
    const tcp_conns t(run.data(), 6, nullptr, 0);
    EXPECT(t.bits() == 4);
    for (size_t c = 0; c < run.size(); ++c) EXPECT(t.lookup(run[c]) == static_cast<int64_t>(c));
    for (const auto& c : others) EXPECT(t.lookup(c) == -1);
    EXPECT(tcp_conns::slot(run[0], 32) % 16 == 15 && tcp_conns::slot(run[0], 17) % 16 == 15);
    // a map has no duplicate keys
    sccsum_tcp_conns* h = nullptr;
    const sccsum_tcp_conn twice[3] = {run[0], run[1], run[0]};
    const uint16_t ports_twice[3] = {80, 443, 80};
    EXPECT(sccsum_tcp_conns_create_host(twice, 3, nullptr, 0, &h) == SCCSUM_EINVAL && h == nullptr);
    EXPECT(sccsum_tcp_conns_create_host(twice, 2, ports_twice, 3, &h) == SCCSUM_EINVAL && h == nullptr);
    EXPECT(sccsum_tcp_conns_create_host(nullptr, 2, nullptr, 0, &h) == SCCSUM_EINVAL);
    EXPECT(sccsum_tcp_conns_create_host(twice, 2, nullptr, 1, &h) == SCCSUM_EINVAL);
    EXPECT(sccsum_tcp_conns_create_host(twice, SCCSUM_TCP_MAX_CONNS + 1, nullptr, 0, &h) == SCCSUM_EINVAL);
    EXPECT(sccsum_tcp_conns_create_host(twice, 2, ports_twice, 65537, &h) == SCCSUM_EINVAL);
    EXPECT(sccsum_tcp_conns_create_host(twice, 2, nullptr, 0, nullptr) == SCCSUM_EINVAL);
    EXPECT(sccsum_tcp_conns_lookup(nullptr, 1, 2, 3, 4) == -1 && sccsum_tcp_conns_listening(nullptr, 80) == 0);
    EXPECT(sccsum_tcp_conns_count(nullptr) == 0 && sccsum_tcp_conns_bits(nullptr) == 0);
    EXPECT(sccsum_tcp_conns_destroy(nullptr) == SCCSUM_OK);
    bool threw = false;
    try {
        const tcp_conns dup(twice, 3, nullptr, 0);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT(threw);
    return entries;
}

template <typename T>
T* at(uintptr_t a) {
    return reinterpret_cast<T*>(a);
}

constexpr uintptr_t p = 0x10000;  // a dummy device address: nothing is dereferenced before the checks are done

int refused = 0;

// the class call must throw (the library refused it); a host-only table's valid call is refused with ENODEV, which throws too
template <typename F>
void refuses(F&& f, const char* what, int line) {
    ++refused;
    try {
        f();
        std::printf("NOT REFUSED %s (line %d)\n", what, line);
        ++bad;
    } catch (const std::runtime_error&) {
    }
}
#define REFUSES(x) refuses([&] { x; }, #x, __LINE__)

void calls() {
    const sccsum_tcp_conn one{1, 2, 3, 4};
    const uint16_t port = 80;
    const tcp_conns t(&one, 1, &port, 1);
    const tcp_rx rx(t, 0x0A000001u);
    EXPECT(rx.workspace(0) == sccsum_tcp_rx_workspace(0, 1) && rx.workspace(5000) == sccsum_tcp_rx_workspace(5000, 1));
    EXPECT(rx.workspace(5000) % 16 == 0 && rx.workspace(5000) >= 56u * 5000u + 256u * 4u * 5u);
    EXPECT(tcp_rx::taken(7, 0) == 0 && tcp_rx::taken(7, 59) == 2 && tcp_rx::taken(7, 60) == 3 &&
           tcp_rx::taken(7, 1 << 20) == 7);
    const device_packet_batch ip{at<void>(p), 1 << 20, at<uint64_t>(p), at<uint32_t>(p), 8, 0};
    tcp_rx::outputs o;
    o.first = at<uint32_t>(p), o.order = at<uint32_t>(p), o.seg = at<sccsum_tcp_seg>(p), o.src = at<uint32_t>(p);
    o.run_conn = at<uint32_t>(p), o.run_first = at<uint32_t>(p), o.rst = at<void>(p), o.rst_dst = at<uint32_t>(p);
    o.total = at<uint64_t>(p);
    // direct C call: everything valid, only the host-only table's missing device copy stops it
    EXPECT(sccsum_tcp_rx(ip.bytes, ip.bytes_len, ip.off, ip.len, ip.n, at<uint8_t>(p), 3, 0x1C, 1, t.get(), nullptr, 8, 0,
                         nullptr, o.first, o.order, o.seg, o.src, o.run_conn, o.run_first, o.rst, o.rst_dst, o.total,
                         at<void>(p), nullptr) == SCCSUM_ENODEV);
    REFUSES(rx.run(ip, at<uint8_t>(p), nullptr, 8, o, at<void>(p), nullptr));   // ENODEV
    REFUSES(rx.run(ip, at<uint8_t>(p), nullptr, 9, o, at<void>(p), nullptr));   // n > nbatch without an index
    REFUSES(rx.run(ip, at<uint8_t>(p), nullptr, 8, o, at<void>(p + 8), nullptr));
    REFUSES(rx.run(ip, at<uint8_t>(p), nullptr, 8, o, at<void>(p), nullptr, 0x100));
    REFUSES(rx.run(ip, nullptr, nullptr, 8, o, at<void>(p), nullptr));
    for (int k = 0; k < 9; ++k) {
        tcp_rx::outputs b = o;
        switch (k) {
        case 0: b.first = nullptr; break;
        case 1: b.order = at<uint32_t>(p + 2); break;
        case 2: b.seg = at<sccsum_tcp_seg>(p + 4); break;
        case 3: b.src = nullptr; break;
        case 4: b.run_conn = nullptr; break;
        case 5: b.run_first = at<uint32_t>(p + 2); break;
        case 6: b.rst = at<void>(p + 2); break;
        case 7: b.rst_dst = nullptr; break;
        default: b.total = at<uint64_t>(p + 4); break;
        }
        ++refused;
        if (sccsum_tcp_rx(ip.bytes, ip.bytes_len, ip.off, ip.len, ip.n, at<uint8_t>(p), 3, 0x1C, 1, t.get(), nullptr, 8, 0,
                          nullptr, b.first, b.order, b.seg, b.src, b.run_conn, b.run_first, b.rst, b.rst_dst, b.total,
                          at<void>(p), nullptr) != SCCSUM_EINVAL) {
            std::printf("NOT REFUSED tcp_rx output %d\n", k);
            ++bad;
        }
    }
    const tcp_rx odd(t, 1, 2);  // an unknown flag
    REFUSES(odd.run(ip, at<uint8_t>(p), nullptr, 8, o, at<void>(p), nullptr));

    tcp_tx::outputs s;
    s.l4_off = at<uint64_t>(p), s.l4_len = at<uint32_t>(p), s.sum_len = at<uint32_t>(p), s.seed = at<uint32_t>(p);
    s.tso_seg = at<uint16_t>(p), s.needs_csum = at<uint8_t>(p), s.status = at<uint8_t>(p);
    for (const sccsum_tcp_opts& bad_opts : {sccsum_tcp_opts{1, 67, 0}, sccsum_tcp_opts{1, 65536, 0}, sccsum_tcp_opts{1, 1500, 4}}) {
        const tcp_tx tx(bad_opts);
        REFUSES(tx.run(at<void>(p), 1 << 20, at<uint64_t>(p), at<uint32_t>(p), at<sccsum_tcp_out>(p), 8, s, nullptr));
    }
    const tcp_tx tx({1, 1500, SCCSUM_TCP_CSUM_OFFLOAD | SCCSUM_TCP_TSO});
    EXPECT(tx.opts().mtu == 1500);
    REFUSES(tx.run(at<void>(p), 1 << 20, at<uint64_t>(p + 4), at<uint32_t>(p), at<sccsum_tcp_out>(p), 8, s, nullptr));
    REFUSES(tx.run(at<void>(p), 1 << 20, at<uint64_t>(p), nullptr, at<sccsum_tcp_out>(p), 8, s, nullptr));
    REFUSES(tx.run(at<void>(p), 1 << 20, at<uint64_t>(p), at<uint32_t>(p), at<sccsum_tcp_out>(p + 2), 8, s, nullptr));
    REFUSES(tx.run(at<void>(p), 1 << 20, at<uint64_t>(p), at<uint32_t>(p), nullptr, 8, s, nullptr));
    REFUSES(tx.run(at<void>(p), 1 << 20, at<uint64_t>(p), at<uint32_t>(p), at<sccsum_tcp_out>(p), uint64_t(1) << 32, s, nullptr));
    for (int k = 0; k < 7; ++k) {
        tcp_tx::outputs b = s;
        switch (k) {
        case 0: b.l4_off = at<uint64_t>(p + 4); break;
        case 1: b.l4_len = nullptr; break;
        case 2: b.sum_len = at<uint32_t>(p + 2); break;
        case 3: b.seed = nullptr; break;
        case 4: b.tso_seg = at<uint16_t>(p + 1); break;
        case 5: b.needs_csum = nullptr; break;
        default: b.status = nullptr; break;
        }
        REFUSES(tx.run(at<void>(p), 1 << 20, at<uint64_t>(p), at<uint32_t>(p), at<sccsum_tcp_out>(p), 8, b, nullptr));
    }
}

}  // namespace

int main() {
    std::mt19937 rng(16);
    const size_t entries = tables(rng);
    calls();
    if (bad) {
        std::printf("tcp_host: %d FAILED\n", bad);
        return 1;
    }
    std::printf("tcp_host: OK (%zu table entries against a map, %d calls refused)\n", entries, refused);
    return 0;
}
