// Host-only program over the link-layer C calls and their C++ classes
// (seastar/net/ip_checksum_batch.hh: arp_table, eth_rx, eth_tx): the ARP
// table's build and lookup against a std::map fed the same entries (later
// duplicates win, keys 0 and 255.255.255.255, keys that share a home slot and
// wrap past the last slot), the classes' workspace() against the C calls, and
// every argument error, which the library reports before any device work.
// No launch is made: it runs without a device.  tests/test_eth_host.py builds
// it against the library and, with eth.hip compiled in, under ASan + UBSan.
// Prints "eth_host: OK (...)" and exits 0; a failure names itself, exit 1.
#include <seastar/net/ip_checksum_batch.hh>

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

// Every key of `want` and some absent ones through the table.
void same_as_map(const arp_table& t, const std::map<uint32_t, uint64_t>& want, std::mt19937& rng) {
    for (const auto& kv : want) {
        uint64_t mac = ~uint64_t(0);
        EXPECT(t.lookup(kv.first, &mac) && mac == kv.second);
    }
    for (int k = 0; k < 1000; ++k) {
        const uint32_t ip = rng();
        uint64_t mac = 0x1234;
        const bool hit = t.lookup(ip, &mac);
        const auto it = want.find(ip);
        EXPECT(hit == (it != want.end()));
        EXPECT(hit ? mac == it->second : mac == 0x1234);
    }
}

size_t tables(std::mt19937& rng) {
    size_t entries = 0;
    for (uint32_t n : {0u, 1u, 7u, 8u, 9u, 100u, 5000u}) {
        std::vector<sccsum_arp_entry> e;
        std::map<uint32_t, uint64_t> want;
        for (uint32_t i = 0; i < n; ++i) {
            // few distinct keys: many duplicates, the later one must win
            const uint32_t ip = i == 0 ? 0u : i == 1 ? 0xFFFFFFFFu : 0x0A000000u + rng() % (n / 2 + 1);
            const uint64_t mac = (uint64_t(rng()) << 16 | (rng() & 0xFFFFu)) & 0xFFFFFFFFFFFFull;
            e.push_back({ip, static_cast<uint32_t>(rng()), mac});  // pad is ignored
            want[ip] = mac;
        }
        arp_table t(e.data(), n);
        uint32_t bits = 4;
        while ((uint64_t(1) << bits) < 2 * uint64_t(n)) ++bits;
        EXPECT(t.bits() == bits);
        same_as_map(t, want, rng);
        entries += n;
    }
    // twelve keys whose home is the last slot but one: the probes wrap past the end
    const uint32_t bits = 5;
    std::vector<sccsum_arp_entry> e;
    std::map<uint32_t, uint64_t> want;
    for (uint32_t ip = 1; e.size() < 12; ++ip) {
        if (arp_table::slot(ip, bits) != (1u << bits) - 2) continue;
        e.push_back({ip, 0, uint64_t(ip) * 0x10001u});
        want[ip] = uint64_t(ip) * 0x10001u;
    }
    arp_table t(e.data(), static_cast<uint32_t>(e.size()));
    EXPECT(t.bits() == bits);
    same_as_map(t, want, rng);
    EXPECT(arp_table::slot(1, 32) == UINT32_MAX && arp_table::slot(1, 0) == 0);
    return entries + e.size();
}

int refused = 0;

void einval(int rc, const char* what, int line) {
    ++refused;
    if (rc != SCCSUM_EINVAL) {
        std::printf("NOT REFUSED %s -> %d (line %d)\n", what, rc, line);
        ++bad;
    }
}
#define REFUSED(x) einval((x), #x, __LINE__)

template <typename T>
T* at(uintptr_t a) {
    return reinterpret_cast<T*>(a);
}

void argument_errors() {
    const sccsum_arp_entry one[1] = {{1, 0, 2}};
    const sccsum_arp_entry wide[2] = {{1, 0, 2}, {3, 0, uint64_t(1) << 48}};
    sccsum_arp_table* t = nullptr;
    REFUSED(sccsum_arp_table_create(0, one, 1, nullptr));
    REFUSED(sccsum_arp_table_create(0, nullptr, 1, &t));
    REFUSED(sccsum_arp_table_create(0, wide, 2, &t));
    REFUSED(sccsum_arp_table_create(0, one, SCCSUM_ARP_MAX_ENTRIES + 1, &t));
    REFUSED(sccsum_arp_table_create_host(one, 1, nullptr));
    REFUSED(sccsum_arp_table_create_host(nullptr, 1, &t));
    REFUSED(sccsum_arp_table_create_host(wide, 2, &t));
    EXPECT(sccsum_arp_table_create(-1, one, 1, &t) != SCCSUM_OK && t == nullptr);
    uint64_t mac = 0;
    EXPECT(sccsum_arp_table_lookup(nullptr, 1, &mac) == 0);
    EXPECT(sccsum_arp_table_destroy(nullptr) == SCCSUM_OK && sccsum_arp_table_bits(nullptr) == 0);

    // dummy device addresses: nothing is dereferenced before the checks are done
    const uintptr_t p = 0x10000;
    const uint16_t protos[9] = {0x0800, 0x0806, 1, 2, 3, 4, 5, 6, 7};
    const uint16_t twice[2] = {0x0800, 0x0800};
    auto rx = [&](const uint16_t* pr, uint32_t k, uint64_t n, uintptr_t off, uintptr_t first, uintptr_t order,
                  uintptr_t l3_off, uintptr_t l3_len, uintptr_t mac_, uintptr_t ws) {
        return sccsum_eth_rx(at<void>(p), 1 << 20, at<uint64_t>(off), at<uint32_t>(p), n, pr, k, nullptr,
                             at<uint32_t>(first), at<uint32_t>(order), at<uint64_t>(l3_off), at<uint32_t>(l3_len),
                             at<uint64_t>(mac_), at<void>(ws), nullptr);
    };
    REFUSED(rx(nullptr, 2, 8, p, p, p, p, p, p, p));
    REFUSED(rx(protos, 0, 8, p, p, p, p, p, p, p));
    REFUSED(rx(protos, 9, 8, p, p, p, p, p, p, p));
    REFUSED(rx(twice, 2, 8, p, p, p, p, p, p, p));
    REFUSED(rx(protos, 2, uint64_t(1) << 32, p, p, p, p, p, p, p));
    REFUSED(rx(protos, 2, 8, 0, p, p, p, p, p, p));
    REFUSED(rx(protos, 2, 8, p + 4, p, p, p, p, p, p));
    REFUSED(rx(protos, 2, 8, p, 0, p, p, p, p, p));
    REFUSED(rx(protos, 2, 8, p, p + 2, p, p, p, p, p));
    REFUSED(rx(protos, 2, 8, p, p, 0, p, p, p, p));
    REFUSED(rx(protos, 2, 8, p, p, p + 2, p, p, p, p));
    REFUSED(rx(protos, 2, 8, p, p, p, 0, p, p, p));
    REFUSED(rx(protos, 2, 8, p, p, p, p + 4, p, p, p));
    REFUSED(rx(protos, 2, 8, p, p, p, p, 0, p, p));
    REFUSED(rx(protos, 2, 8, p, p, p, p, p + 2, p, p));
    REFUSED(rx(protos, 2, 8, p, p, p, p, p, 0, p));
    REFUSED(rx(protos, 2, 8, p, p, p, p, p, p + 4, p));
    REFUSED(rx(protos, 2, 8, p, p, p, p, p, p, 0));
    REFUSED(rx(protos, 2, 8, p, p, p, p, p, p, p + 8));
    REFUSED(rx(protos, 2, 0, 0, 0, 0, 0, 0, 0, p));  // n == 0 still writes d_first
    REFUSED(sccsum_eth_rx(nullptr, 64, at<uint64_t>(p), at<uint32_t>(p), 8, protos, 2, nullptr, at<uint32_t>(p),
                          at<uint32_t>(p), at<uint64_t>(p), at<uint32_t>(p), at<uint64_t>(p), at<void>(p), nullptr));

    auto learn = [&](uint64_t n, uint32_t need, uint32_t reject, uintptr_t off, uintptr_t len, uintptr_t st,
                     uintptr_t mac_, uintptr_t rec, uintptr_t count, uintptr_t ws) {
        return sccsum_arp_learn_records(at<void>(p), 1 << 20, at<uint64_t>(off), at<uint32_t>(len), at<uint8_t>(st), need,
                                        reject, at<uint64_t>(mac_), n, 1, 2, nullptr, at<sccsum_arp_rec>(rec),
                                        at<uint32_t>(count), at<void>(ws), nullptr);
    };
    REFUSED(learn(uint64_t(1) << 31, 1, 12, p, p, p, p, p, p, p));
    REFUSED(learn(8, 0x100, 12, p, p, p, p, p, p, p));
    REFUSED(learn(8, 1, 0x100, p, p, p, p, p, p, p));
    REFUSED(learn(8, 1, 12, 0, p, p, p, p, p, p));
    REFUSED(learn(8, 1, 12, p + 4, p, p, p, p, p, p));
    REFUSED(learn(8, 1, 12, p, 0, p, p, p, p, p));
    REFUSED(learn(8, 1, 12, p, p + 2, p, p, p, p, p));
    REFUSED(learn(8, 1, 12, p, p, 0, p, p, p, p));
    REFUSED(learn(8, 1, 12, p, p, p, 0, p, p, p));
    REFUSED(learn(8, 1, 12, p, p, p, p + 4, p, p, p));
    REFUSED(learn(8, 1, 12, p, p, p, p, 0, p, p));
    REFUSED(learn(8, 1, 12, p, p, p, p, p + 4, p, p));
    REFUSED(learn(8, 1, 12, p, p, p, p, p, 0, p));
    REFUSED(learn(8, 1, 12, p, p, p, p, p, p + 2, p));
    REFUSED(learn(8, 1, 12, p, p, p, p, p, p, 0));
    REFUSED(learn(8, 1, 12, p, p, p, p, p, p, p + 8));
    REFUSED(learn(0, 1, 12, 0, 0, 0, 0, 0, 0, p));  // n == 0 still writes *d_count

    arp_table host_only(one, 1);
    const sccsum_eth_opts good = {0x020000000001ull, 0x0A000001u, 0xFFFFFF00u, 0x0A0000FEu, 0x0800};
    sccsum_eth_opts wide_mac = good;
    wide_mac.hw_address |= uint64_t(1) << 48;
    struct send_args {
        const sccsum_eth_opts* opts;
        const sccsum_arp_table* table;
        uint64_t n, frames, cap;
        uintptr_t dst, dgram_first, desc, first, off, len, eth, desc_out, first_out, off_out, len_out, frame_src, status,
            unresolved, total, ws;
    };
    const send_args ok = {&good, host_only.get(), 8, 9, 1 << 20, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p};
    auto send = [&](const send_args& a) {
        return sccsum_eth_send(a.opts, a.table, at<uint32_t>(a.dst), at<uint32_t>(a.dgram_first), a.n,
                               at<sccsum_gather_desc>(a.desc), at<uint32_t>(a.first), at<uint64_t>(a.off),
                               at<uint32_t>(a.len), a.frames, a.cap, at<uint8_t>(a.eth),
                               at<sccsum_gather_desc>(a.desc_out), at<uint32_t>(a.first_out), at<uint64_t>(a.off_out),
                               at<uint32_t>(a.len_out), at<uint32_t>(a.frame_src), at<uint8_t>(a.status),
                               at<sccsum_eth_unresolved>(a.unresolved), at<uint64_t>(a.total), at<void>(a.ws), nullptr);
    };
    // the valid call gets past every argument check: only the table's missing device copy stops it
    EXPECT(send(ok) == SCCSUM_ENODEV);
    send_args a = ok;
    a.opts = nullptr;
    REFUSED(send(a));
    a = ok, a.opts = &wide_mac;
    REFUSED(send(a));
    a = ok, a.table = nullptr;
    REFUSED(send(a));
    a = ok, a.n = uint64_t(1) << 32;
    REFUSED(send(a));
    a = ok, a.frames = uint64_t(1) << 31;
    REFUSED(send(a));
    a = ok, a.cap = uint64_t(1) << 32;
    REFUSED(send(a));
    a = ok, a.dgram_first = 0;  // one frame per datagram, but 9 frames for 8 datagrams
    REFUSED(send(a));
    uintptr_t send_args::*const required[] = {&send_args::dst,       &send_args::first,     &send_args::off,
                                              &send_args::len,       &send_args::eth,       &send_args::desc_out,
                                              &send_args::first_out, &send_args::off_out,   &send_args::len_out,
                                              &send_args::frame_src, &send_args::status,    &send_args::unresolved,
                                              &send_args::total,     &send_args::ws};
    for (auto m : required) {
        a = ok, a.*m = 0;
        REFUSED(send(a));
    }
    struct {
        uintptr_t send_args::*m;
        uintptr_t by;
    } const aligned[] = {{&send_args::dst, 2},       {&send_args::dgram_first, 2}, {&send_args::desc, 4},
                         {&send_args::first, 2},     {&send_args::off, 4},         {&send_args::len, 2},
                         {&send_args::desc_out, 4},  {&send_args::first_out, 2},   {&send_args::off_out, 4},
                         {&send_args::len_out, 2},   {&send_args::frame_src, 2},   {&send_args::unresolved, 4},
                         {&send_args::total, 4},     {&send_args::ws, 8}};
    for (const auto& c : aligned) {
        a = ok, a.*c.m = p + c.by;
        REFUSED(send(a));
    }
    a = ok, a.n = 0, a.frames = 0, a.total = 0;  // n == 0 still writes d_total
    REFUSED(send(a));
    // a host-only table given to learn is refused after the argument checks as well
    EXPECT(sccsum_arp_learn_records(at<void>(p), 64, at<uint64_t>(p), at<uint32_t>(p), at<uint8_t>(p), 1, 12,
                                    at<uint64_t>(p), 8, 1, 2, host_only.get(), at<sccsum_arp_rec>(p), at<uint32_t>(p),
                                    at<void>(p), nullptr) == SCCSUM_ENODEV);
}

void wrappers() {
    for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(1024), uint64_t(1025), uint64_t(1) << 20, uint64_t(3000001)}) {
        EXPECT(eth_rx::workspace(n) == sccsum_eth_rx_workspace(n) && eth_rx::workspace(n) % 16 == 0);
        EXPECT(eth_rx::learn_workspace(n) == sccsum_arp_learn_workspace(n) && eth_rx::learn_workspace(n) % 16 == 0);
        EXPECT(eth_tx::workspace(n) == sccsum_eth_send_workspace(n) && eth_tx::workspace(n) % 16 == 0);
        EXPECT(eth_rx::workspace(n) >= 16 && eth_rx::learn_workspace(n) >= 16 && eth_tx::workspace(n) >= 16);
    }
    const eth_rx rx({0x0800, 0x0806});
    EXPECT(rx.protos() == 2);
    bool threw = false;
    try {
        const eth_rx none({});
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT(threw);
    const eth_tx tx({0x020000000001ull, 1, 2, 3, 0x0800});
    EXPECT(tx.opts().gw == 3 && tx.opts().eth_proto == 0x0800);
    threw = false;
    try {
        // the classes turn the C calls' codes into exceptions
        rx.run(device_packet_batch{nullptr, 0, nullptr, nullptr, 0, 0}, eth_rx::outputs{}, nullptr, nullptr);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    EXPECT(threw);
}

}  // namespace

int main() {
    std::mt19937 rng(15);
    const size_t entries = tables(rng);
    argument_errors();
    wrappers();
    if (bad) return 1;
    std::printf("eth_host: OK (%zu entries, %d refused)\n", entries, refused);
    return 0;
}
