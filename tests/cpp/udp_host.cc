// Host-only program over the UDP-layer C calls and their C++ classes
// (seastar/net/ip_checksum_batch.hh: udp_ports, udp_rx, udp_tx): the port
// table's lookup against a std::map over all 65 536 ports, the classes'
// workspace() and taken() against the C calls, and every argument error,
// which the library reports before any device work.  No launch is made: it
// runs without a device.  tests/test_udp_host.py builds it against the
// library and, with udp.hip compiled in, under ASan + UBSan.
// Prints "udp_host: OK (...)" and exits 0; a failure names itself, exit 1.
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

size_t tables(std::mt19937& rng) {
    size_t bound = 0;
    for (uint32_t c : {0u, 1u, 2u, 64u, 65u, 251u, 252u}) {
        std::map<uint16_t, int> want;
        std::vector<uint16_t> ports;
        while (ports.size() < c) {
            const uint16_t p = ports.empty() ? 0 : ports.size() == 1 ? 65535 : static_cast<uint16_t>(rng());
            if (want.count(p)) continue;
            want[p] = static_cast<int>(ports.size());
            ports.push_back(p);
        }
        const udp_ports t(ports.data(), c);
        EXPECT(t.channels() == c);
        for (uint32_t p = 0; p < 65536; ++p) {
            const auto it = want.find(static_cast<uint16_t>(p));
            EXPECT(t.lookup(static_cast<uint16_t>(p)) == (it == want.end() ? -1 : it->second));
        }
        bound += c;
    }
    EXPECT(sccsum_udp_ports_lookup(nullptr, 53) == -1 && sccsum_udp_ports_channels(nullptr) == 0);
    EXPECT(sccsum_udp_ports_destroy(nullptr) == SCCSUM_OK);
    return bound;
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

constexpr uintptr_t p = 0x10000;  // a dummy device address: nothing is dereferenced before the checks are done

struct rx_args {
    const sccsum_udp_ports* ports;
    uint64_t nbatch, n;
    uint32_t need, reject;
    uintptr_t bytes, off, len, status, index, cls, first, order, pay_off, pay_len, src, sport, ws;
};

int rx(const rx_args& a) {
    return sccsum_udp_rx(at<void>(a.bytes), 1 << 20, at<uint64_t>(a.off), at<uint32_t>(a.len), a.nbatch,
                         at<uint8_t>(a.status), a.need, a.reject, 0x0A000001u, a.ports, at<uint32_t>(a.index), a.n,
                         at<uint8_t>(a.cls), at<uint32_t>(a.first), at<uint32_t>(a.order), at<uint64_t>(a.pay_off),
                         at<uint32_t>(a.pay_len), at<uint32_t>(a.src), at<uint16_t>(a.sport), at<void>(a.ws), nullptr);
}

struct reasm_args {
    const sccsum_udp_ports* ports;
    uint64_t m, nrec;
    uint32_t need, reject;
    uintptr_t desc, dfirst, doff, dlen, dhead, rec, l4_status, cls, first, order, pay_len, src, sport, ws;
};

int reasm(const reasm_args& a) {
    return sccsum_udp_rx_reasm(at<sccsum_gather_desc>(a.desc), at<uint32_t>(a.dfirst), at<uint64_t>(a.doff),
                               at<uint32_t>(a.dlen), at<uint32_t>(a.dhead), a.m, at<sccsum_frag_rec>(a.rec), a.nrec,
                               at<uint8_t>(a.l4_status), a.need, a.reject, 0x0A000001u, a.ports, at<uint8_t>(a.cls),
                               at<uint32_t>(a.first), at<uint32_t>(a.order), at<uint32_t>(a.pay_len), at<uint32_t>(a.src),
                               at<uint16_t>(a.sport), at<void>(a.ws), nullptr);
}

struct send_args {
    const sccsum_udp_opts* opts;
    uint64_t n;
    uintptr_t bytes, off, len, dst, dport, sport, l4_off, l4_len, sum_len, seed, proto, needs_csum, status;
};

int send(const send_args& a) {
    return sccsum_udp_send(a.opts, at<void>(a.bytes), 1 << 20, at<uint64_t>(a.off), at<uint32_t>(a.len),
                           at<uint32_t>(a.dst), at<uint16_t>(a.dport), at<uint16_t>(a.sport), a.n, at<uint64_t>(a.l4_off),
                           at<uint32_t>(a.l4_len), at<uint32_t>(a.sum_len), at<uint32_t>(a.seed), at<uint8_t>(a.proto),
                           at<uint8_t>(a.needs_csum), at<uint8_t>(a.status), nullptr);
}

template <typename A, size_t N>
void each_null(const A& ok, int (*call)(const A&), uintptr_t A::*const (&members)[N]) {
    for (auto m : members) {
        A a = ok;
        a.*m = 0;
        REFUSED(call(a));
    }
}

template <typename A>
struct misalign {
    uintptr_t A::*m;
    uintptr_t by;
};

template <typename A, size_t N>
void each_misaligned(const A& ok, int (*call)(const A&), const misalign<A> (&members)[N]) {
    for (const auto& c : members) {
        A a = ok;
        a.*c.m = p + c.by;
        REFUSED(call(a));
    }
}

void argument_errors() {
    const uint16_t two[2] = {53, 10000};
    const uint16_t twice[3] = {53, 10000, 53};
    std::vector<uint16_t> many(SCCSUM_UDP_MAX_CHANNELS + 1);
    for (size_t k = 0; k < many.size(); ++k) many[k] = static_cast<uint16_t>(k);
    sccsum_udp_ports* t = nullptr;
    REFUSED(sccsum_udp_ports_create(0, two, 2, nullptr));
    REFUSED(sccsum_udp_ports_create(0, nullptr, 2, &t));
    REFUSED(sccsum_udp_ports_create(0, twice, 3, &t));
    REFUSED(sccsum_udp_ports_create(0, many.data(), SCCSUM_UDP_MAX_CHANNELS + 1, &t));
    REFUSED(sccsum_udp_ports_create_host(two, 2, nullptr));
    REFUSED(sccsum_udp_ports_create_host(nullptr, 1, &t));
    REFUSED(sccsum_udp_ports_create_host(twice, 3, &t));
    REFUSED(sccsum_udp_ports_create_host(many.data(), SCCSUM_UDP_MAX_CHANNELS + 1, &t));
    EXPECT(t == nullptr);
    EXPECT(sccsum_udp_ports_create(-1, two, 2, &t) != SCCSUM_OK && t == nullptr);

    const udp_ports host_only(two, 2);
    const sccsum_udp_ports* const h = host_only.get();

    // udp_rx: the valid call gets past every argument check; only the table's missing device copy stops it
    const rx_args rok = {h, 8, 8, 1, 0x1C, p, p, p, p, p, p, p, p, p, p, p, p, p};
    EXPECT(rx(rok) == SCCSUM_ENODEV);
    rx_args a = rok;
    a.ports = nullptr;
    REFUSED(rx(a));
    a = rok, a.need = 0x100;
    REFUSED(rx(a));
    a = rok, a.reject = 0x100;
    REFUSED(rx(a));
    a = rok, a.n = uint64_t(1) << 32;
    REFUSED(rx(a));
    a = rok, a.nbatch = uint64_t(1) << 32;
    REFUSED(rx(a));
    a = rok, a.index = 0, a.n = 9;  // without an index the call's frames are a prefix of the batch
    REFUSED(rx(a));
    a = rok, a.n = 9;               // with one it may be longer than the batch
    EXPECT(rx(a) == SCCSUM_ENODEV);
    a = rok, a.index = 0, a.cls = 0;  // both optional
    EXPECT(rx(a) == SCCSUM_ENODEV);
    uintptr_t rx_args::*const rx_required[] = {&rx_args::bytes, &rx_args::off,   &rx_args::len,     &rx_args::status,
                                               &rx_args::first, &rx_args::order, &rx_args::pay_off, &rx_args::pay_len,
                                               &rx_args::src,   &rx_args::sport, &rx_args::ws};
    each_null(rok, rx, rx_required);
    const misalign<rx_args> rx_aligned[] = {{&rx_args::off, 4},     {&rx_args::len, 2},   {&rx_args::index, 2},
                                            {&rx_args::first, 2},   {&rx_args::order, 2}, {&rx_args::pay_off, 4},
                                            {&rx_args::pay_len, 2}, {&rx_args::src, 2},   {&rx_args::sport, 1},
                                            {&rx_args::ws, 8}};
    each_misaligned(rok, rx, rx_aligned);
    a = rok, a.n = 0, a.nbatch = 0, a.first = 0;  // n == 0 still writes d_first
    REFUSED(rx(a));
    a = rok, a.n = 0, a.nbatch = 0, a.ws = 0;
    REFUSED(rx(a));

    // udp_rx_reasm
    const reasm_args mok = {h, 8, 20, 1, 8, p, p, p, p, p, p, p, p, p, p, p, p, p, p};
    EXPECT(reasm(mok) == SCCSUM_ENODEV);
    reasm_args b = mok;
    b.ports = nullptr;
    REFUSED(reasm(b));
    b = mok, b.need = 0x100;
    REFUSED(reasm(b));
    b = mok, b.reject = 0x100;
    REFUSED(reasm(b));
    b = mok, b.m = uint64_t(1) << 31;
    REFUSED(reasm(b));
    b = mok, b.nrec = uint64_t(1) << 31;
    REFUSED(reasm(b));
    b = mok, b.l4_status = 0;  // masks without the status they test
    REFUSED(reasm(b));
    b = mok, b.l4_status = 0, b.need = 0, b.reject = 0, b.cls = 0;
    EXPECT(reasm(b) == SCCSUM_ENODEV);
    uintptr_t reasm_args::*const reasm_required[] = {
        &reasm_args::desc,  &reasm_args::dfirst, &reasm_args::doff,    &reasm_args::dlen, &reasm_args::dhead,
        &reasm_args::rec,   &reasm_args::first,  &reasm_args::order,   &reasm_args::pay_len,
        &reasm_args::src,   &reasm_args::sport,  &reasm_args::ws};
    each_null(mok, reasm, reasm_required);
    const misalign<reasm_args> reasm_aligned[] = {
        {&reasm_args::desc, 4},  {&reasm_args::dfirst, 2}, {&reasm_args::doff, 4},    {&reasm_args::dlen, 2},
        {&reasm_args::dhead, 2}, {&reasm_args::rec, 4},    {&reasm_args::first, 2},   {&reasm_args::order, 2},
        {&reasm_args::pay_len, 2}, {&reasm_args::src, 2},  {&reasm_args::sport, 1},   {&reasm_args::ws, 8}};
    each_misaligned(mok, reasm, reasm_aligned);
    b = mok, b.m = 0, b.first = 0;  // m == 0 still writes d_first
    REFUSED(reasm(b));

    // udp_send: no table; the valid call is stopped only by the missing device (or runs nothing: n == 0)
    const sccsum_udp_opts good = {0x0A000001u, 1500, SCCSUM_UDP_CSUM_OFFLOAD | SCCSUM_UDP_UFO};
    const send_args sok = {&good, 8, p, p, p, p, p, p, p, p, p, p, p, p, p};
    send_args s = sok;
    s.opts = nullptr;
    REFUSED(send(s));
    for (uint32_t mtu : {0u, 67u, 65536u}) {
        const sccsum_udp_opts o = {1, mtu, 0};
        s = sok, s.opts = &o;
        REFUSED(send(s));
    }
    const sccsum_udp_opts flags = {1, 1500, 4};
    s = sok, s.opts = &flags;
    REFUSED(send(s));
    s = sok, s.n = uint64_t(1) << 32;
    REFUSED(send(s));
    uintptr_t send_args::*const send_required[] = {
        &send_args::bytes,  &send_args::off,    &send_args::len,     &send_args::dst,  &send_args::dport,
        &send_args::sport,  &send_args::l4_off, &send_args::l4_len,  &send_args::sum_len,
        &send_args::seed,   &send_args::needs_csum, &send_args::status};
    each_null(sok, send, send_required);
    const misalign<send_args> send_aligned[] = {{&send_args::off, 4},     {&send_args::len, 2},    {&send_args::dst, 2},
                                                {&send_args::dport, 1},   {&send_args::sport, 1},  {&send_args::l4_off, 4},
                                                {&send_args::l4_len, 2},  {&send_args::sum_len, 2}, {&send_args::seed, 2}};
    each_misaligned(sok, send, send_aligned);
}

void wrappers() {
    for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(1024), uint64_t(1025), uint64_t(1) << 20, uint64_t(3000001)}) {
        EXPECT(udp_rx::workspace(n) == sccsum_udp_rx_workspace(n) && udp_rx::workspace(n) % 16 == 0);
        EXPECT(udp_rx::reassembled_workspace(n) == sccsum_udp_rx_reasm_workspace(n));
        EXPECT(udp_rx::workspace(n) >= 16 + 253 * 4 * ((n + 1023) / 1024));
    }
    EXPECT(udp_rx::taken(0, 1024) == 0 && udp_rx::taken(5, 1024) == 5 && udp_rx::taken(1024, 1024) == 1024 &&
           udp_rx::taken(1100, 1024) == 1024 && udp_rx::taken(7, 0) == 0);
    const uint16_t two[2] = {53, 10000};
    const udp_ports ports(two, 2);
    const udp_rx rx_(ports, 0x0A000001u);
    EXPECT(rx_.host_address() == 0x0A000001u);
    const udp_tx tx({0x0A000001u, 576, SCCSUM_UDP_UFO});
    EXPECT(tx.opts().mtu == 576 && tx.opts().flags == SCCSUM_UDP_UFO);
    int threw = 0;
    try {
        const uint16_t twice[2] = {53, 53};
        const udp_ports none(twice, 2);
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        // the classes turn the C calls' codes into exceptions
        rx_.run(device_packet_batch{nullptr, 0, nullptr, nullptr, 0, 0}, nullptr, nullptr, 0, udp_rx::outputs{}, nullptr,
                nullptr);
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        rx_.run_reassembled(udp_rx::datagrams{}, nullptr, udp_rx::outputs{}, nullptr, nullptr);
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        const udp_tx small({1, 20, 0});
        small.run(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, udp_tx::outputs{}, nullptr);
    } catch (const std::runtime_error&) {
        ++threw;
    }
    EXPECT(threw == 4);
}

}  // namespace

int main() {
    std::mt19937 rng(16);
    const size_t bound = tables(rng);
    argument_errors();
    wrappers();
    if (bad) return 1;
    std::printf("udp_host: OK (%zu ports bound, %d refused)\n", bound, refused);
    return 0;
}
