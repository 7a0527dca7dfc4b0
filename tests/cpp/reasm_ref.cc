// The REFERENCE's own packet_merger (include/seastar/net/packet-util.hh, used
// where it lies) fed the fragment sequences of a case file; it prints the map
// after every merge, for tests/test_reasm_ref.py to compare with the Python
// restatement (tests/reasm_model.py) byte for byte, and for
// tests/golden/make_reasm.py to record.
//
// Case file: one sequence per line, "n off len off len ...".  Record r's
// payload byte p is payload_byte(r, p) below (the same in reasm_model.py).
// Output: per sequence a line "S n", then per merge a line
// "nseg beg len hex ...", hex = "-" for an empty segment.
#include <seastar/net/packet-util.hh>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

// Test-only definitions of the two out-of-line symbols the header needs (the
// reference's own translation units want fmt, absent here).
namespace seastar::internal {
[[noreturn]] void assert_fail(const char* msg, const char* file, int line, const char* func) {
    std::fprintf(stderr, "assertion failed: %s at %s:%d (%s)\n", msg, file, line, func);
    std::abort();
}
}  // namespace seastar::internal

namespace seastar::net {
// The merger linearizes whole packets only: every byte copied, in order, into
// one new fragment that the packet then owns.
void packet::linearize(size_t at_frag, size_t desired_size) {
    if (at_frag != 0 || desired_size != len()) std::abort();
    const size_t n = len();
    char* const flat = new char[n ? n : 1];
    size_t at = 0;
    for (auto&& f : fragments()) {
        for (size_t k = 0; k < f.size; ++k) flat[at++] = f.base[k];
    }
    *this = packet(fragment{flat, n}, make_deleter([flat] { delete[] flat; }));
}
}  // namespace seastar::net

using namespace seastar;

struct test_tag {};

static unsigned char payload_byte(uint64_t rec, uint64_t pos) {
    return static_cast<unsigned char>((((rec + 1) * 2654435761ull + pos * 40503ull) >> 7) & 0xFF);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    size_t nseq = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        size_t n = 0;
        if (!(ls >> n)) continue;
        std::printf("S %zu\n", n);
        net::packet_merger<uint32_t, test_tag> m;
        std::vector<std::vector<char>> bufs(n);
        for (size_t r = 0; r < n; ++r) {
            uint32_t off = 0, len = 0;
            if (!(ls >> off >> len)) return 3;
            bufs[r].resize(len ? len : 1);
            for (uint32_t p = 0; p < len; ++p) bufs[r][p] = static_cast<char>(payload_byte(r, p));
            m.merge(off, net::packet(net::fragment{bufs[r].data(), len}, make_deleter([] {})));
            std::printf("%zu", m.map.size());
            for (auto& [beg, pkt] : m.map) {
                std::printf(" %u %u ", unsigned(beg), unsigned(pkt.len()));
                if (pkt.len() == 0) std::printf("-");
                for (auto&& f : pkt.fragments()) {
                    for (size_t k = 0; k < f.size; ++k) std::printf("%02x", static_cast<unsigned char>(f.base[k]));
                }
            }
            std::printf("\n");
        }
        ++nseq;
    }
    std::fprintf(stderr, "reasm_ref: %zu sequences\n", nseq);
    return 0;
}
