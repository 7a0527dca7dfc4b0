// Native host program over the C++ classes tx_sender, rx_steering and
// rx_reassembler (seastar/net/ip_checksum_batch.hh): each forwards 10-20
// arguments, many of one type, to a C call that the Python tests pin.  Here the
// wrapper and the C call it forwards to run on the same inputs into two
// separately poisoned sets of outputs (64 guard bytes behind each array, the
// workspaces poisoned too), every optional argument given, and every array must
// be byte-equal: a swapped or dropped argument shows.  The inputs span a tile
// edge of every kernel: a send tile + 300 UDP datagrams cut at MTU 68, their
// wire frames (gathered, shuffled) through the frames call, the steering, the
// fragment records and the reassembly.  Prints OK and exits 0; a mismatch
// prints the array's name and exits 1.
#include <hip/hip_runtime.h>
#include <sccsum_diag.h>
#include <seastar/net/ip_checksum_batch.hh>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
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

// What a send writes, with room for `frames` frames of n datagrams.
struct send_set {
    dev_array hdr, desc, first, out_off, out_len, dgram_first, status, total, ws;
    send_set(uint64_t frames, uint64_t n)
        : hdr(20 * frames), desc(32 * frames), first(4 * (frames + 1)), out_off(8 * frames), out_len(4 * frames),
          dgram_first(4 * (n + 1)), status(n), total(24), ws(tx_sender::workspace(n), 0x5A) {}
};

struct steer_set {
    dev_array cpu, order, first, ws;
    steer_set(uint64_t n, uint32_t ncpu, uint64_t ws_bytes) : cpu(n), order(4 * n), first(4 * (ncpu + 2)), ws(ws_bytes, 0x5A) {}
};

struct records_set {
    dev_array rec, count, ws;
    explicit records_set(uint64_t n) : rec(32 * n), count(4), ws(rx_reassembler::workspace(n), 0x5A) {}
};

struct reasm_set {
    dev_array desc, dgram_first, dgram_off, dgram_len, dgram_seed, dgram_head, dgram_last, dgram_hash, pending, host,
        rec_state, total, ws;
    explicit reasm_set(uint64_t m)
        : desc(16 * m), dgram_first(4 * (m + 1)), dgram_off(8 * m), dgram_len(4 * m), dgram_seed(4 * m),
          dgram_head(4 * m), dgram_last(4 * m), dgram_hash(4 * m), pending(32 * m), host(32 * m), rec_state(m),
          total(32), ws(rx_reassembler::workspace(m), 0x5A) {}
    sccsum_reasm_out out() const {
        return sccsum_reasm_out{desc.as<sccsum_gather_desc>(), dgram_first.as<uint32_t>(), dgram_off.as<uint64_t>(),
                                dgram_len.as<uint32_t>(),      dgram_seed.as<uint32_t>(),  dgram_head.as<uint32_t>(),
                                dgram_last.as<uint32_t>(),     dgram_hash.as<uint32_t>(),  pending.as<sccsum_frag_rec>(),
                                host.as<sccsum_frag_rec>(),    rec_state.as<uint8_t>(),    total.as<uint64_t>()};
    }
};

void c_ok(int rc, const char* what) {
    if (rc != SCCSUM_OK) {
        std::printf("%s: %s\n", what, sccsum_strerror(rc));
        std::exit(2);
    }
}

}  // namespace

int main() {
    batch_checksummer shard(0);  // binds this thread to device 0 (sccsum_init)
    hipStream_t stream;
    HIP_OK(hipStreamCreate(&stream));
    std::mt19937 rng(0x5CA22);
    static const uint8_t key[40] = {0xd1, 0x81, 0xc6, 0x2c, 0xf7, 0xf4, 0xdb, 0x5b, 0x19, 0x83, 0xa2, 0xfc, 0x94, 0x3e,
                                    0x1a, 0xdb, 0xd9, 0x38, 0x9e, 0x6b, 0xd1, 0x03, 0x9c, 0x2c, 0xa7, 0x44, 0x99, 0xad,
                                    0x59, 0x3d, 0x56, 0xd9, 0xf3, 0x25, 0x3c, 0x06, 0x2a, 0xdc, 0x1f, 0xfc};
    const uint32_t me = 0xC0A80A63, other_host = 0xC0A80B63, my_src = 0xC0A80A01, mtu = 68;

    // ---- tx_sender::run: a send tile + 300 UDP datagrams of 0..200 bytes, ids, L4 values, a frame cap that cuts
    const uint32_t n = uint32_t(sccsum_send_tile_datagrams()) + 300;
    std::vector<uint8_t> l4_host;
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> len(n), dst(n);
    std::vector<uint8_t> proto(n, 17);
    std::vector<uint16_t> ids(n), l4sum(n);
    const tx_sender tx(my_src, mtu);
    uint64_t need_frames = 0;
    for (uint32_t i = 0; i < n; ++i) {
        len[i] = rng() % 201;
        off[i] = l4_host.size() + rng() % 3;
        l4_host.resize(off[i] + len[i]);
        for (uint32_t k = 0; k < len[i]; ++k) l4_host[off[i] + k] = uint8_t(rng());
        dst[i] = rng() % 2 ? me : other_host;
        ids[i] = uint16_t(i * 7 + 1);  // one key per datagram (n < 65536 / 7)
        l4sum[i] = uint16_t(rng());
        need_frames += tx.plan(len[i], 17).frames;
    }
    l4_host.resize(l4_host.size() + 16);
    const uint64_t max_frames = need_frames - 5, max_bytes = 0xFFFFFFF0ull;  // the last datagrams do not fit
    if (need_frames <= uint64_t(sccsum_send_emit_tile_frames()) + 5) {
        std::printf("the frames do not span an emit tile\n");
        return 2;
    }
    dev_array d_l4(l4_host.size()), d_off(8 * n), d_len(4 * n), d_dst(4 * n), d_proto(n), d_ids(2 * n), d_l4sum(2 * n);
    upload(d_l4, l4_host);
    upload(d_off, off);
    upload(d_len, len);
    upload(d_dst, dst);
    upload(d_proto, proto);
    upload(d_ids, ids);
    upload(d_l4sum, l4sum);
    const device_packet_batch l4{d_l4.p, l4_host.size(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), n, 200};
    send_set sa(max_frames, n), sb(max_frames, n);
    tx_sender::outputs o;
    o.hdr = sa.hdr.p;
    o.desc = sa.desc.as<sccsum_gather_desc>();
    o.first = sa.first.as<uint32_t>();
    o.out_off = sa.out_off.as<uint64_t>();
    o.out_len = sa.out_len.as<uint32_t>();
    o.dgram_first = sa.dgram_first.as<uint32_t>();
    o.status = sa.status.p;
    o.total = sa.total.as<uint64_t>();
    tx.run(l4, d_dst.as<uint32_t>(), d_proto.p, d_ids.as<uint16_t>(), d_l4sum.as<uint16_t>(), max_frames, max_bytes, o,
           sa.ws.p, stream);
    const sccsum_send_opts opts{my_src, mtu, SCCSUM_SEND_L4};
    c_ok(sccsum_ipv4_send(&opts, d_l4.p, l4_host.size(), d_off.as<uint64_t>(), d_len.as<uint32_t>(),
                          d_dst.as<uint32_t>(), d_proto.p, d_ids.as<uint16_t>(), d_l4sum.as<uint16_t>(), n, max_frames,
                          max_bytes, sb.hdr.p, sb.desc.as<sccsum_gather_desc>(), sb.first.as<uint32_t>(),
                          sb.out_off.as<uint64_t>(), sb.out_len.as<uint32_t>(), sb.dgram_first.as<uint32_t>(),
                          sb.status.p, sb.total.as<uint64_t>(), sb.ws.p, stream),
         "sccsum_ipv4_send");
    shard.sync(stream);
    same("send.hdr", sa.hdr, sb.hdr);
    same("send.first", sa.first, sb.first);
    same("send.out_off", sa.out_off, sb.out_off);
    same("send.out_len", sa.out_len, sb.out_len);
    same("send.dgram_first", sa.dgram_first, sb.dgram_first);
    same("send.status", sa.status, sb.status);
    same("send.total", sa.total, sb.total);
    uint64_t total[3];
    HIP_OK(hipMemcpy(total, sa.total.p, 24, hipMemcpyDeviceToHost));
    uint32_t frames = 0;
    HIP_OK(hipMemcpy(&frames, sa.dgram_first.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost));
    if (total[0] != need_frames || total[2] >= n || total[2] + 6 < n || frames == 0 || frames > max_frames) {
        std::printf("MISMATCH send.total: %llu frames needed (%llu planned), %llu datagrams emitted, %u frames\n",
                    (unsigned long long)total[0], (unsigned long long)need_frames, (unsigned long long)total[2], frames);
        ++bad;
    }
    {
        // the descriptors: the header records' src as offsets from their own d_hdr, everything else as it is
        std::vector<uint8_t> ha = sa.desc.host(), hb = sb.desc.host();
        for (uint32_t f = 0; f < frames; ++f) {
            uint64_t a, b;
            std::memcpy(&a, ha.data() + 32 * size_t(f), 8);
            std::memcpy(&b, hb.data() + 32 * size_t(f), 8);
            a -= reinterpret_cast<uint64_t>(sa.hdr.p);
            b -= reinterpret_cast<uint64_t>(sb.hdr.p);
            if (a != b || a != 20ull * f) {
                std::printf("MISMATCH send.desc (header source of frame %u)\n", f);
                ++bad;
                break;
            }
            std::memset(ha.data() + 32 * size_t(f), 0, 8);
            std::memset(hb.data() + 32 * size_t(f), 0, 8);
        }
        if (ha != hb) {
            std::printf("MISMATCH send.desc\n");
            ++bad;
        }
    }

    // ---- the wire frames, packed and shuffled, through the frames call: status and hashes
    std::vector<uint64_t> f_off(frames);
    std::vector<uint32_t> f_len(frames);
    HIP_OK(hipMemcpy(f_off.data(), sa.out_off.p, 8 * size_t(frames), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(f_len.data(), sa.out_len.p, 4 * size_t(frames), hipMemcpyDeviceToHost));
    const uint64_t wire_bytes = f_off[frames - 1] + f_len[frames - 1];
    dev_array d_wire(wire_bytes + 16), d_foff(8 * size_t(frames)), d_flen(4 * size_t(frames)), d_st(frames),
        d_hash(4 * size_t(frames));
    c_ok(sccsum_gather(sa.desc.as<sccsum_gather_desc>(), 2ull * frames, d_wire.p, stream), "sccsum_gather");
    std::vector<uint32_t> perm(frames);
    std::iota(perm.begin(), perm.end(), 0u);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<uint64_t> p_off(frames);
    std::vector<uint32_t> p_len(frames);
    for (uint32_t f = 0; f < frames; ++f) {
        p_off[f] = f_off[perm[f]];
        p_len[f] = f_len[perm[f]];
    }
    upload(d_foff, p_off);
    upload(d_flen, p_len);
    const device_packet_batch wire{d_wire.p, wire_bytes, d_foff.as<uint64_t>(), d_flen.as<uint32_t>(), frames, mtu};
    shard.ipv4_frames_rss(wire, key, sizeof(key), SCCSUM_RSS_DISPATCH, nullptr, d_st.p, d_hash.as<uint32_t>(), stream);

    // ---- rx_steering::run: 5 shards, the fragments dropped by their status bit
    {
        const uint32_t cpus[5] = {0, 1, 2, 3, 4};
        const float weights[5] = {1.0f, 2.0f, 0.5f, 1.5f, 1.0f};
        uint8_t reta[128];
        rx_steering::build_reta(cpus, weights, 5, reta);
        const sccsum_steer_map map = {5, 1, 0, 0, nullptr, reta, nullptr};
        rx_steering steer(0, map);
        if (frames <= uint32_t(sccsum_steer_tile_packets())) {
            std::printf("the frames do not span a steering tile\n");
            return 2;
        }
        steer_set a(frames, 5, steer.workspace(frames)), b(frames, 5, steer.workspace(frames));
        const uint32_t need = SCCSUM_ST_OK, reject = SCCSUM_ST_IPFRAG;
        steer.run(SCCSUM_STEER_HASH2CPU, 0, d_hash.as<uint32_t>(), d_st.p, need, reject, frames, a.cpu.p,
                  a.order.as<uint32_t>(), a.first.as<uint32_t>(), a.ws.p, stream);
        sccsum_steer* raw = nullptr;
        c_ok(sccsum_steer_create(0, &map, &raw), "sccsum_steer_create");
        c_ok(sccsum_steer_run(raw, SCCSUM_STEER_HASH2CPU, 0, d_hash.as<uint32_t>(), d_st.p, need, reject, frames,
                              b.cpu.p, b.order.as<uint32_t>(), b.first.as<uint32_t>(), b.ws.p, stream),
             "sccsum_steer_run");
        shard.sync(stream);
        c_ok(sccsum_steer_destroy(raw), "sccsum_steer_destroy");
        same("steer.cpu", a.cpu, b.cpu);
        same("steer.order", a.order, b.order);
        same("steer.first", a.first, b.first);
        uint32_t first[7];
        HIP_OK(hipMemcpy(first, a.first.p, sizeof(first), hipMemcpyDeviceToHost));
        if (first[6] != frames || first[5] == 0 || first[5] == frames) {  // some steered, some dropped
            std::printf("MISMATCH steer.first: %u steered of %u\n", first[5], first[6]);
            ++bad;
        }
        steer.close();
    }

    // ---- rx_reassembler::records: this host's fragments, masks and tag given
    const rx_reassembler rx(me);
    records_set ra(frames), rb(frames);
    const uint32_t need = SCCSUM_ST_OK | SCCSUM_ST_IPFRAG, reject = SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE;
    const uint32_t tag = 0xBEEF0001u;
    rx.records(wire, d_st.p, tag, ra.rec.as<sccsum_frag_rec>(), ra.count.as<uint32_t>(), ra.ws.p, stream, need, reject);
    c_ok(sccsum_ipv4_frag_records(d_wire.p, wire_bytes, d_foff.as<uint64_t>(), d_flen.as<uint32_t>(), d_st.p, need,
                                  reject, frames, me, tag, rb.rec.as<sccsum_frag_rec>(), rb.count.as<uint32_t>(),
                                  rb.ws.p, stream),
         "sccsum_ipv4_frag_records");
    shard.sync(stream);
    same("records.rec", ra.rec, rb.rec);
    same("records.count", ra.count, rb.count);
    uint32_t m = 0;
    HIP_OK(hipMemcpy(&m, ra.count.p, 4, hipMemcpyDeviceToHost));
    if (m <= uint32_t(sccsum_reasm_scan_tile_records()) || m >= frames) {
        std::printf("MISMATCH records.count: %u records of %u frames do not span a scan tile\n", m, frames);
        return 1;
    }

    // ---- rx_reassembler::run: a capacity that leaves datagrams pending, the key, every output
    reasm_set qa(m), qb(m);
    const uint64_t cap = 40000;
    const sccsum_reasm_out out_a = qa.out(), out_b = qb.out();
    rx.run(ra.rec.as<sccsum_frag_rec>(), m, cap, key, sizeof(key), out_a, qa.ws.p, stream);
    c_ok(sccsum_ipv4_reasm(ra.rec.as<sccsum_frag_rec>(), m, cap, key, sizeof(key), &out_b, qb.ws.p, stream),
         "sccsum_ipv4_reasm");
    shard.sync(stream);
    same("reasm.desc", qa.desc, qb.desc);
    same("reasm.dgram_first", qa.dgram_first, qb.dgram_first);
    same("reasm.dgram_off", qa.dgram_off, qb.dgram_off);
    same("reasm.dgram_len", qa.dgram_len, qb.dgram_len);
    same("reasm.dgram_seed", qa.dgram_seed, qb.dgram_seed);
    same("reasm.dgram_head", qa.dgram_head, qb.dgram_head);
    same("reasm.dgram_last", qa.dgram_last, qb.dgram_last);
    same("reasm.dgram_hash", qa.dgram_hash, qb.dgram_hash);
    same("reasm.pending", qa.pending, qb.pending);
    same("reasm.host", qa.host, qb.host);
    same("reasm.rec_state", qa.rec_state, qb.rec_state);
    same("reasm.total", qa.total, qb.total);
    uint64_t rt[4];
    HIP_OK(hipMemcpy(rt, qa.total.p, 32, hipMemcpyDeviceToHost));
    if (rt[0] == 0 || rt[1] <= rt[0] || rt[2] == 0 || rt[1] + rt[2] + rt[3] != m) {
        std::printf("MISMATCH reasm.total: %llu datagrams, %llu descriptors, %llu pending, %llu host of %u records\n",
                    (unsigned long long)rt[0], (unsigned long long)rt[1], (unsigned long long)rt[2],
                    (unsigned long long)rt[3], m);
        ++bad;
    }
    HIP_OK(hipStreamDestroy(stream));
    if (bad) {
        std::printf("FAILED: %d arrays differ\n", bad);
        return 1;
    }
    std::printf("rxtx_gpu: OK (%u datagrams sent as %u frames, steered, %u fragment records, %llu datagrams "
                "reassembled, %llu records pending: wrappers and C calls byte-equal)\n",
                n, frames, m, (unsigned long long)rt[0], (unsigned long long)rt[2]);
    return 0;
}
