// seastar::net::tx_sender's host arithmetic (plan) against values the test
// passes in (tests/test_send_host.py writes the case file):
//   P <mtu> <flags> <proto> <l4_len> <want frames> <want bytes>   one datagram's plan
//   X <mtu> <flags>                                               options plan() must refuse
#include <seastar/net/ip_checksum_batch.hh>

#include <cstdio>
#include <fstream>
#include <string>

using seastar::net::tx_sender;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string tag;
    unsigned long plans = 0, refused = 0;
    while (in >> tag) {
        if (tag == "P") {
            uint32_t mtu = 0, flags = 0, proto = 0, len = 0, want_frames = 0;
            uint64_t want_bytes = 0;
            in >> mtu >> flags >> proto >> len >> want_frames >> want_bytes;
            if (!in) return 2;
            const tx_sender tx(0x0A000001u, mtu, flags);
            const tx_sender::plan_result a = tx.plan(len, static_cast<uint8_t>(proto));
            const tx_sender::plan_result b = tx_sender::plan(tx.opts(), len, static_cast<uint8_t>(proto));
            if (a.frames != want_frames || a.out_bytes != want_bytes || b.frames != a.frames ||
                b.out_bytes != a.out_bytes) {
                std::printf("plan: mtu %u flags %u proto %u len %u: got %u frames %llu bytes, want %u / %llu\n", mtu,
                            flags, proto, len, a.frames, static_cast<unsigned long long>(a.out_bytes), want_frames,
                            static_cast<unsigned long long>(want_bytes));
                return 1;
            }
            ++plans;
        } else if (tag == "X") {
            uint32_t mtu = 0, flags = 0;
            in >> mtu >> flags;
            if (!in) return 2;
            try {
                (void)tx_sender(1, mtu, flags).plan(100, 17);
                std::printf("plan accepted bad options (mtu %u flags %u)\n", mtu, flags);
                return 1;
            } catch (const std::runtime_error&) {
                ++refused;
            }
        } else {
            return 2;
        }
    }
    if (tx_sender::workspace(0) == 0 || tx_sender::workspace(1000) % 16 != 0) return 1;
    std::printf("send_host: OK (%lu plans, %lu refused)\n", plans, refused);
    return 0;
}
