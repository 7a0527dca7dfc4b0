// seastar::net::rx_steering's host arithmetic (build_reta, dest) against
// values the test passes in (tests/test_steer_host.py writes the case file):
//   M <ncpu> <hw_queues> <table_bits> <redir_size> <has_set>   a map, then its tables:
//     redir_size redir entries, hw_queues * 128 reta entries, has_set ? hw_queues flags
//   D <mode> <src_cpu> <hash> <want>                            one hash through the last map
//   R <n> { <cpu> <weight as float bits> } x n  <128 wanted entries>
//   X <ncpu> <hw_queues> <table_bits> <redir_size>              a map dest() must refuse
#include <seastar/net/ip_checksum_batch.hh>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

using seastar::net::rx_steering;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::vector<uint8_t> redir, reta, set;
    sccsum_steer_map map{};
    std::string tag;
    unsigned long dests = 0, retas = 0, refused = 0;
    while (in >> tag) {
        if (tag == "M") {
            unsigned has_set = 0;
            in >> map.ncpu >> map.hw_queues >> map.table_bits >> map.redir_size >> has_set;
            redir.assign(map.redir_size, 0);
            reta.assign(size_t(map.hw_queues) * 128, 0);
            set.assign(has_set ? map.hw_queues : 0, 0);
            unsigned v = 0;
            for (auto& x : redir) { in >> v; x = static_cast<uint8_t>(v); }
            for (auto& x : reta) { in >> v; x = static_cast<uint8_t>(v); }
            for (auto& x : set) { in >> v; x = static_cast<uint8_t>(v); }
            map.redir = redir.empty() ? nullptr : redir.data();
            map.sw_reta = reta.data();
            map.sw_reta_set = set.empty() ? nullptr : set.data();
        } else if (tag == "D") {
            int mode = 0;
            uint32_t src = 0, hash = 0, want = 0;
            in >> mode >> src >> hash >> want;
            const uint32_t got = rx_steering::dest(map, mode, src, hash);
            if (got != want) {
                std::printf("dest: mode %d src %u hash %08x: got %u, want %u\n", mode, src, hash, got, want);
                return 1;
            }
            ++dests;
        } else if (tag == "R") {
            uint32_t n = 0;
            in >> n;
            std::vector<uint32_t> cpus(n);
            std::vector<float> weights(n);
            for (uint32_t i = 0; i < n; ++i) {
                uint32_t bits = 0;
                in >> cpus[i] >> bits;
                std::memcpy(&weights[i], &bits, 4);
            }
            uint8_t got[128];
            std::memset(got, 0xEE, sizeof(got));
            rx_steering::build_reta(cpus.data(), weights.data(), n, got);
            for (int i = 0; i < 128; ++i) {
                unsigned want = 0;
                in >> want;
                if (got[i] != want) {
                    std::printf("build_reta: case %lu entry %d: got %u, want %u\n", retas, i, unsigned(got[i]), want);
                    return 1;
                }
            }
            ++retas;
        } else if (tag == "X") {
            sccsum_steer_map bad{};
            uint8_t row[128] = {};
            in >> bad.ncpu >> bad.hw_queues >> bad.table_bits >> bad.redir_size;
            bad.sw_reta = row;
            bad.redir = bad.redir_size ? row : nullptr;
            try {
                (void)rx_steering::dest(bad, SCCSUM_STEER_HASH2CPU, 0, 1);
                std::printf("dest accepted a bad map (%u %u %u %u)\n", bad.ncpu, bad.hw_queues, bad.table_bits,
                            bad.redir_size);
                return 1;
            } catch (const std::runtime_error&) {
                ++refused;
            }
        } else {
            return 2;
        }
        if (!in) return 2;
    }
    std::printf("steer_host: OK (%lu dests, %lu retas, %lu refused)\n", dests, retas, refused);
    return 0;
}
