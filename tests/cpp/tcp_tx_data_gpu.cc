// Native host program over the C++ class tcp_tx_data
// (seastar/net/ip_checksum_batch.hh): run() forwards 18 arguments, many of one
// type, four of them taken from a queues struct and seven from an outputs
// struct, to a C call that the Python tests pin.  Here the wrapper and the C
// call run on the same inputs into two separately poisoned sets of outputs (64
// guard bytes behind each array, the workspaces poisoned too), and every array
// must be byte-equal: a swapped or dropped argument, or a field mapped to the
// wrong parameter, shows.  The input: 1 300 connections with queues of 0 to 6
// buffers, some of no bytes, windows that close early, small cwnds, every
// seventh connection not eligible, once without and once with a capacity that
// cuts the last connections off.  The descriptors of the first round are then
// gathered and every segment's bytes compared with its connection's stream.
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

struct out_set {
    dev_array run, off, len, out, seg_first, desc, total, ws;
    out_set(uint64_t nconns, uint64_t max_segs, uint64_t nbuf, uint64_t ws_bytes)
        : run(sizeof(sccsum_tcp_snd_run) * nconns), off(8 * max_segs), len(4 * max_segs),
          out(sizeof(sccsum_tcp_out) * max_segs), seg_first(4 * (max_segs + 1)),
          desc(sizeof(sccsum_gather_desc) * (max_segs + nbuf)), total(8 * 4), ws(ws_bytes, 0x5A) {}
    tcp_tx_data::outputs outputs() const {
        tcp_tx_data::outputs o;
        o.run = run.as<sccsum_tcp_snd_run>();
        o.off = off.as<uint64_t>();
        o.len = len.as<uint32_t>();
        o.out = out.as<sccsum_tcp_out>();
        o.seg_first = seg_first.as<uint32_t>();
        o.desc = desc.as<sccsum_gather_desc>();
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
    std::mt19937 rng(89);

    constexpr uint32_t kConns = 1300, kHeadroom = 24;
    std::vector<sccsum_tcp_snd> snd(kConns);
    std::vector<uint32_t> buf_len, buf_first(kConns + 1);
    std::vector<uint64_t> buf_at;   // a buffer's first byte in the blob
    std::vector<uint8_t> blob;
    for (uint32_t c = 0; c < kConns; ++c) {
        sccsum_tcp_snd& s = snd[c];
        s = sccsum_tcp_snd{};
        s.dst = 0x0A000100 + c;
        s.next = c == 5 ? 0xFFFFFF00u : static_cast<uint32_t>(rng());
        s.una = s.next - rng() % 2000;
        s.window = c % 5 == 0 ? 2500 : 60000;
        s.cwnd = c % 11 == 0 ? 100 + rng() % 300 : 14600;
        s.rcv_next = static_cast<uint32_t>(rng());
        s.sport = static_cast<uint16_t>(1024 + c);
        s.dport = 80;
        s.mss = c % 3 ? 1460 : 536;
        s.wnd = static_cast<uint16_t>(rng());
        s.flags = static_cast<uint8_t>((c % 7 == 6 ? 0 : SCCSUM_TCP_SND_ELIGIBLE) | (c & 1 ? SCCSUM_TCP_SND_RTX_ARMED : 0));
        buf_first[c] = static_cast<uint32_t>(buf_len.size());
        const uint32_t nb = rng() % 7;
        for (uint32_t k = 0; k < nb; ++k) {
            const uint32_t n = rng() % 4 == 0 ? 0 : 1 + rng() % 2500;
            buf_len.push_back(n);
            buf_at.push_back(blob.size());
            for (uint32_t b = 0; b < n; ++b) blob.push_back(static_cast<uint8_t>(rng()));
            blob.push_back(0xEE);   // a gap between the buffers
        }
    }
    const uint64_t nbuf = buf_len.size();
    buf_first[kConns] = static_cast<uint32_t>(nbuf);
    dev_array d_blob(blob.size()), d_snd(sizeof(sccsum_tcp_snd) * kConns), d_src(8 * nbuf), d_len(4 * nbuf),
        d_first(4 * (kConns + 1));
    std::vector<uint64_t> src(nbuf);
    for (uint64_t j = 0; j < nbuf; ++j) src[j] = reinterpret_cast<uint64_t>(d_blob.p) + buf_at[j];
    upload(d_blob, blob);
    upload(d_snd, snd);
    upload(d_src, src);
    upload(d_len, buf_len);
    upload(d_first, buf_first);

    const sccsum_tcp_tx_opts opts{0x0A000001, 1500, 65535, kHeadroom, 0};
    const tcp_tx_data cut(opts);
    tcp_tx_data::queues q;
    q.src = d_src.as<uint64_t>();
    q.len = d_len.as<uint32_t>();
    q.first = d_first.as<uint32_t>();
    q.nbuf = nbuf;
    const uint64_t ws_bytes = tcp_tx_data::workspace(kConns, nbuf);
    if (ws_bytes != sccsum_tcp_tx_data_workspace(kConns, nbuf)) {
        std::printf("MISMATCH workspace\n");
        ++bad;
    }
    constexpr uint64_t kMaxSegs = 16384;
    uint64_t needed = 0, emitted[2] = {0, 0};
    for (int round = 0; round < 2; ++round) {
        // the second round with a capacity that cuts the last connections off
        const uint64_t max_bytes = round == 0 ? 0xFFFFFFFFull : needed - 5000;
        out_set a(kConns, kMaxSegs, nbuf, ws_bytes), b(kConns, kMaxSegs, nbuf, ws_bytes);
        cut.run(d_snd.as<sccsum_tcp_snd>(), kConns, q, kMaxSegs, max_bytes, a.outputs(), a.ws.p, stream);
        const tcp_tx_data::outputs ob = b.outputs();
        const int rc = sccsum_tcp_tx_data(&opts, d_snd.as<sccsum_tcp_snd>(), kConns, q.src, q.len, q.first, nbuf, kMaxSegs,
                                          max_bytes, ob.run, ob.off, ob.len, ob.out, ob.seg_first, ob.desc, ob.total,
                                          b.ws.p, stream);
        if (rc != SCCSUM_OK) {
            std::printf("sccsum_tcp_tx_data: %s\n", sccsum_strerror(rc));
            return 2;
        }
        HIP_OK(hipStreamSynchronize(stream));
        same("run", a.run, b.run);
        same("off", a.off, b.off);
        same("len", a.len, b.len);
        same("out", a.out, b.out);
        same("seg_first", a.seg_first, b.seg_first);
        same("desc", a.desc, b.desc);
        same("total", a.total, b.total);
        uint64_t total[4];
        HIP_OK(hipMemcpy(total, a.total.p, sizeof(total), hipMemcpyDeviceToHost));
        std::vector<sccsum_tcp_snd_run> runs(kConns);
        HIP_OK(hipMemcpy(runs.data(), a.run.p, sizeof(sccsum_tcp_snd_run) * kConns, hipMemcpyDeviceToHost));
        uint64_t segs = 0, bytes = 0, capped = 0;
        for (const sccsum_tcp_snd_run& r : runs) {
            if (r.seg_first != segs) {
                std::printf("MISMATCH run.seg_first\n");
                ++bad;
                break;
            }
            segs += r.segs;
            bytes += r.bytes + uint64_t(kHeadroom) * r.segs;
            capped += r.stop == SCCSUM_TCP_STOP_CAPACITY;
        }
        if (total[0] != segs || total[1] != bytes || segs < kConns / 2 || segs > kMaxSegs ||
            runs[6].stop != SCCSUM_TCP_STOP_INELIGIBLE || (round == 0) != (capped == 0) ||
            (round == 0 ? total[3] != bytes : total[3] != needed || bytes > max_bytes)) {
            std::printf("MISMATCH total values: %llu segments, %llu bytes, %llu needed, %llu connections cut\n",
                        static_cast<unsigned long long>(total[0]), static_cast<unsigned long long>(total[1]),
                        static_cast<unsigned long long>(total[3]), static_cast<unsigned long long>(capped));
            ++bad;
        }
        needed = total[3];
        emitted[round] = total[0];
        if (round != 0) continue;
        // the gather: every segment's bytes are its connection's stream bytes
        dev_array staging(total[1]);
        const int grc = sccsum_gather(a.desc.as<sccsum_gather_desc>(), total[2], staging.p, stream);
        if (grc != SCCSUM_OK) {
            std::printf("sccsum_gather: %s\n", sccsum_strerror(grc));
            return 2;
        }
        HIP_OK(hipStreamSynchronize(stream));
        const std::vector<uint8_t> lay = staging.host();
        std::vector<uint64_t> off(segs);
        std::vector<uint32_t> len(segs);
        HIP_OK(hipMemcpy(off.data(), a.off.p, 8 * segs, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(len.data(), a.len.p, 4 * segs, hipMemcpyDeviceToHost));
        for (uint32_t c = 0; c < kConns && !bad; ++c) {
            std::vector<uint8_t> text;
            for (uint32_t j = buf_first[c]; j < buf_first[c + 1]; ++j) {
                text.insert(text.end(), blob.begin() + buf_at[j], blob.begin() + buf_at[j] + buf_len[j]);
            }
            uint64_t at = 0;
            for (uint64_t f = runs[c].seg_first; f < uint64_t(runs[c].seg_first) + runs[c].segs; ++f) {
                if (at + len[f] > text.size() || off[f] + len[f] > total[1] ||
                    std::memcmp(lay.data() + off[f], text.data() + at, len[f]) != 0) {
                    std::printf("MISMATCH gathered bytes of connection %u\n", c);
                    ++bad;
                    break;
                }
                at += len[f];
            }
            if (at != runs[c].bytes) {
                std::printf("MISMATCH bytes of connection %u\n", c);
                ++bad;
            }
        }
    }
    HIP_OK(hipStreamDestroy(stream));
    if (bad) return 1;
    std::printf("tcp_tx_data_gpu: OK (%u connections, %llu buffers: %llu segments, %llu under the capacity)\n", kConns,
                static_cast<unsigned long long>(nbuf), static_cast<unsigned long long>(emitted[0]),
                static_cast<unsigned long long>(emitted[1]));
    return 0;
}
