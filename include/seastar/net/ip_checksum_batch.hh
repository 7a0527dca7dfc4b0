// seastar/net/ip_checksum_batch.hh — C++ batch interface to the MI355X
// checksum engine (libsccsum, C-ABI in <sccsum.h>), in Seastar's vocabulary.
//
// The per-packet API (<seastar/net/ip_checksum.hh>) stays synchronous and on
// the reactor thread.  This header is what a shard uses to hand a burst of
// packets to its GPU: one launch checksums every packet of the burst.
//
//   per-packet reference call                          batch equivalent
//   ------------------------------------------------   --------------------------------
//   ip_checksum(data, len)           ip_checksum.cc:70-74     sum_spans(batch, nullptr, ...)
//   checksummer + *_pseudo_header_checksum + sum + get        sum_spans(batch, seeds, ...)
//       udp.cc:184-195, tcp.hh:1656-1694, tcp.hh:1004-1016
//   ip.cc:121-127 (IPv4 verify) + tcp.hh:876-883 (TCP verify) ipv4_frames(batch, ...)
//   ip.cc:271-277 (IPv4 generate) + udp/tcp generate          ipv4_frames(batch, ...) on zeroed fields
//   the same, stored into the frames (wire-ready tx)          ipv4_fill(batch, SCCSUM_FILL_IP | SCCSUM_FILL_L4, ...)
//   checksummer::sum(const packet&)  ip_checksum.cc:64-68     spans_desc / ipv4_frames_desc (fragments
//                                                             anywhere the device reads); C-ABI sccsum_fragments
//   tx packets (header fragment + payload fragments), filled   ipv4_fill_desc(...) / burst_queue::set_fill (the
//       where they lie: tcp.hh:1691-1694, udp.cc:184-195          qp::poll_tx hook: wire-ready mbufs at completion)
//   toeplitz_hash(rss_key(), forward_hash)  net.cc:330-341    ipv4_rss(batch, key, ...) / ipv4_frames_rss(...)
//   hash2cpu / forward_dst + forward()  net.hh:287-305,       rx_steering (shard of every packet + the batch's
//       net.cc:330-344, ip.cc:197                                 indices grouped by shard, in arrival order)
//   ipv4::send: the header it prepends and the cut past the    tx_sender (headers + header / payload fragment
//       MTU  ip.cc:100-111, 244-299                               lists for a batch of L4 datagrams; no copy)
//   ipv4 reassembly: frag::merge, packet_merger::merge          rx_reassembler (fragment records, complete datagrams
//       ip.cc:164-220, 412-437, packet-util.hh:45-151              as fragment lists in delivery order; no copy)
//   interface::dispatch_packet, _arp.learn candidates          eth_rx (frames grouped by eth_proto, trimmed;
//       net.cc:324-357, ip.cc:147-149                              the learn records of an IPv4 bucket), arp_table
//   get_l2_dst_address + the interface's eth_hdr               eth_tx (next hop looked up, Ethernet descriptor
//       ip.cc:231-242, net.cc:266-284                              in front of every frame's list; no copy)
//   handle_received_packet's end + ipv4_udp::received          udp_rx (frames / reassembled datagrams grouped by
//       ip.cc:159-162, 222-227, udp.cc:45-53, 164-173              channel, headers trimmed), udp_ports
//   ipv4_udp::send  udp.cc:175-197                             udp_tx (the header in the payload's headroom, the
//                                                                  checksum pass's spans and seeds)
//   per packet as qp::poll_tx / DPDK rx hand them over        burst_queue (host packets, async completion)
//       net.cc:81-105, dpdk.cc:2190-2204
//   a shard's steady stream of bursts, polled like its queues  resident_engine (one grid, steps streamed in;
//       reactor.cc:3543-3550                                   fills too: submit_fill)
//
// Results are network-order uint16 values, exactly what checksummer::get()
// returns; a verify passes when the value is 0.  Errors throw
// std::runtime_error (the C-ABI underneath never throws).
#pragma once

#include <sccsum.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <utility>

#if __cplusplus >= 202002L
#include <span>
#endif

namespace seastar {

namespace net {

namespace detail {

// Every error of the C-ABI becomes "<the call>: <sccsum_strerror>".
inline void check(int rc, const char* what) {
    if (rc != SCCSUM_OK) {
        throw std::runtime_error(std::string(what) + ": " + sccsum_strerror(rc));
    }
}

// The one owner of a C-ABI object: filled through out() by the object's create
// call, destroyed with it; neither copied nor moved.
template <typename T, int (*Destroy)(T*)>
class handle {
    T* _p = nullptr;

public:
    handle() = default;
    handle(const handle&) = delete;
    handle& operator=(const handle&) = delete;
    ~handle() { Destroy(_p); }

    T** out() noexcept { return &_p; }
    T* get() const noexcept { return _p; }
    // destroy now and report what the destructor cannot
    void close(const char* what) {
        T* p = _p;
        _p = nullptr;
        check(Destroy(p), what);
    }
};

}  // namespace detail

// Packets resident in device memory: one byte buffer plus offset/length
// arrays (see <sccsum.h> "Memory contract").
struct device_packet_batch {
    const void* bytes = nullptr;   // 16-byte aligned device pointer
    uint64_t bytes_len = 0;        // valid bytes at `bytes`
    const uint64_t* off = nullptr; // device, n entries
    const uint32_t* len = nullptr; // device, n entries
    uint64_t n = 0;
    uint32_t max_len = 0;          // upper bound of len[] (0 = unknown); tunes the launch only
};

enum class checksum_status : uint8_t {
    ok = SCCSUM_ST_OK,               // spans: result 0; frames: IPv4 header verifies
    l4_ok = SCCSUM_ST_L4_OK,         // frames: TCP/UDP checksum verifies
    malformed = SCCSUM_ST_MALFORMED, // frames: shorter than 20 B / than the IP length, bad ihl
    out_of_range = SCCSUM_ST_RANGE,  // span outside the byte buffer (not read)
    ip_fragment = SCCSUM_ST_IPFRAG,  // frames: MF or offset set — L4 is checked after reassembly (ip.cc:164-220)
};

class batch_checksummer {
    int _device;

public:
    // Binds the calling thread (the shard's reactor thread) to `device`.
    explicit batch_checksummer(int device) : _device(device) { detail::check(sccsum_init(device), "sccsum_init"); }

    int device() const noexcept { return _device; }

    // The pseudo-header partial sum ipv4_traits::{tcp,udp}_pseudo_header_checksum
    // leaves in a fresh checksummer (ip.hh:70-75); host-order addresses, len
    // truncated to 16 bits exactly like the reference's uint16_t parameter.
    static uint32_t pseudo_header_seed(uint32_t src_host, uint32_t dst_host, uint8_t proto, uint16_t len) noexcept {
        return sccsum_pseudo_seed(src_host, dst_host, proto, len);
    }

    // out[i] = checksum of span i, seeded with seeds[i] when seeds != nullptr.
    void sum_spans(const device_packet_batch& b, const uint32_t* d_seeds, uint16_t* d_out, uint8_t* d_status,
                   void* stream) const {
        detail::check(sccsum_spans(b.bytes, b.bytes_len, b.off, b.len, d_seeds, d_out, d_status, b.n, b.max_len,
                                   stream),
                      "sccsum_spans");
    }

    // out2[2i] = IPv4 header checksum, out2[2i+1] = TCP/UDP checksum of frame i.
    // d_out2 may be null when d_status is given: verify only, 1 status byte
    // written per frame (what the reference keeps of the sum, ip.cc:121-127).
    void ipv4_frames(const device_packet_batch& b, uint16_t* d_out2, uint8_t* d_status, void* stream) const {
        detail::check(sccsum_ipv4_frames(b.bytes, b.bytes_len, b.off, b.len, d_out2, d_status, b.n, b.max_len, stream),
                      "sccsum_ipv4_frames");
    }

    // Generate IPv4 header and/or TCP/UDP checksums (ICMP echo replies with
    // SCCSUM_FILL_ICMP_ECHO) and store them into the frames (mode:
    // SCCSUM_FILL_*; d_status and d_out2 may be null: without d_out2 the
    // two passes of SCCSUM_FILL_L4 / SCCSUM_FILL_ICMP_ECHO hand the values over
    // in stream-ordered scratch).  IP fragments get their IPv4 header checksum only.
    void ipv4_fill(const device_packet_batch& b, uint32_t mode, uint16_t* d_out2, uint8_t* d_status,
                   void* stream) const {
        detail::check(sccsum_ipv4_fill(const_cast<void*>(b.bytes), b.bytes_len, b.off, b.len, d_out2, d_status, b.n,
                                       b.max_len, mode, stream),
                      "sccsum_ipv4_fill");
    }

    // RSS: d_hash[i] = toeplitz_hash(key, forward_hash of frame i) (toeplitz.hh:78-98, net.cc:330-341);
    // mode SCCSUM_RSS_DISPATCH or SCCSUM_RSS_REASSEMBLED.  key is host memory
    // (the reference's rss_key_type: 40 or 52 bytes, at least 4).
    void ipv4_rss(const device_packet_batch& b, const uint8_t* key, size_t key_len, int mode, uint32_t* d_hash,
                  uint8_t* d_status, void* stream) const {
        detail::check(sccsum_ipv4_rss(b.bytes, b.bytes_len, b.off, b.len, key, static_cast<uint32_t>(key_len), mode,
                                      d_hash, d_status, b.n, stream),
                      "sccsum_ipv4_rss");
    }

    // ipv4_frames and ipv4_rss in one pass over the bytes.
    void ipv4_frames_rss(const device_packet_batch& b, const uint8_t* key, size_t key_len, int mode,
                         uint16_t* d_out2, uint8_t* d_status, uint32_t* d_hash, void* stream) const {
        detail::check(sccsum_ipv4_frames_rss(b.bytes, b.bytes_len, b.off, b.len, d_out2, d_status, b.n, b.max_len, key,
                                             static_cast<uint32_t>(key_len), mode, d_hash, stream),
                      "sccsum_ipv4_frames_rss");
    }

#if __cplusplus >= 202002L
    // The same with the reference's key type (rss_key_type = std::span<const uint8_t>, toeplitz.hh:49).
    void ipv4_rss(const device_packet_batch& b, std::span<const uint8_t> key, int mode, uint32_t* d_hash,
                  uint8_t* d_status, void* stream) const {
        ipv4_rss(b, key.data(), key.size(), mode, d_hash, d_status, stream);
    }
#endif

    // Packets as fragment lists summed where the fragments lie (HBM, pinned /
    // registered host memory over PCIe, or d_stage for src == nullptr):
    // checksummer::sum(const packet&) (ip_checksum.cc:64-68) without a gather.
    // Packet i is d_desc[d_first[i] .. d_first[i+1]), tiling its bytes from
    // dst_off = d_off[i]; d_len / max_len as in device_packet_batch.
    void spans_desc(const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off,
                    const uint32_t* d_len, uint64_t n, uint32_t max_len, const void* d_stage, const uint32_t* d_seeds,
                    uint16_t* d_out, uint8_t* d_status, void* stream) const {
        detail::check(sccsum_spans_desc(d_desc, d_first, d_off, d_len, d_seeds, d_stage, d_out, d_status, n, max_len,
                                        stream),
                      "sccsum_spans_desc");
    }

    void ipv4_frames_desc(const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off,
                          const uint32_t* d_len, uint64_t n, uint32_t max_len, const void* d_stage, uint16_t* d_out2,
                          uint8_t* d_status, void* stream) const {
        detail::check(sccsum_ipv4_frames_desc(d_desc, d_first, d_off, d_len, d_stage, d_out2, d_status, n, max_len,
                                              stream),
                      "sccsum_ipv4_frames_desc");
    }

    // ipv4_fill on fragment lists: generate and store the checksums where the
    // fragments lie — the memory behind d_desc[].src (d_stage for src ==
    // nullptr) is WRITTEN: device memory or pinned / registered host memory,
    // visible to the host once `stream` is synchronised.  mode: SCCSUM_FILL_*;
    // d_out2 and d_status may be null.  A field may straddle two fragments.
    void ipv4_fill_desc(const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off,
                        const uint32_t* d_len, uint64_t n, uint32_t max_len, uint32_t mode, void* d_stage,
                        uint16_t* d_out2, uint8_t* d_status, void* stream) const {
        detail::check(sccsum_ipv4_fill_desc(d_desc, d_first, d_off, d_len, d_stage, d_out2, d_status, n, max_len, mode,
                                            stream),
                      "sccsum_ipv4_fill_desc");
    }

    void sync(void* stream) const { detail::check(sccsum_sync(stream), "sccsum_sync"); }
};

// Burst queue (<sccsum.h> sccsum_burst_*): packets from HOST memory, handed
// over one at a time as qp::poll_tx and the DPDK rx loop do, batched for the
// GPU and completed through `done(first_ticket, count, results, status)` on
// the polling thread, in submit order.  poll() has pollfn::poll's contract
// (core/internal/poll.hh:26-29: true = did work), so it registers as a poller
// the way qp registers poll_tx (net.cc:109):
//   burst_queue q(gpu, SCCSUM_PIPE_IPV4, 16 << 20, 8192, 50'000, 4, on_done);
//   auto p = reactor::poller::simple([&] { return q.poll(); });
//   q.submit(reinterpret_cast<const sccsum_fragment*>(pkt.fragment_array()), pkt.nr_frags());
// The queue hands `this` to the C-ABI, so it neither copies nor moves.
template <typename Done>
class burst_queue {
    sccsum_burst* _q = nullptr;
    Done _done;

    static void complete(void* self, uint64_t first, uint32_t count, const uint16_t* results, const uint8_t* status) {
        static_cast<burst_queue*>(self)->_done(first, count, results, status);
    }

public:
    burst_queue(int device, int mode, uint64_t batch_bytes, uint32_t batch_packets, uint64_t max_delay_ns, int depth,
                Done done)
        : _done(std::move(done)) {
        detail::check(sccsum_burst_create(device, mode, batch_bytes, batch_packets, max_delay_ns, depth, &complete,
                                          this, &_q),
                      "sccsum_burst_create");
    }
    burst_queue(const burst_queue&) = delete;
    burst_queue& operator=(const burst_queue&) = delete;
    ~burst_queue() { sccsum_burst_destroy(_q); }

    // false: every batch slot is in flight (poll, then submit again)
    bool submit(const sccsum_fragment* frags, uint32_t nfrag, uint32_t seed = 0, uint64_t* ticket = nullptr) {
        const int rc = sccsum_burst_submit(_q, frags, nfrag, seed, ticket);
        if (rc == SCCSUM_EBUSY) return false;
        detail::check(rc, "sccsum_burst_submit");
        return true;
    }
    // zero-copy: fragments in device-readable pinned / registered host memory,
    // untouched until their completion (sccsum_burst_submit_mapped)
    bool submit_mapped(const sccsum_fragment* frags, uint32_t nfrag, uint32_t seed = 0, uint64_t* ticket = nullptr) {
        const int rc = sccsum_burst_submit_mapped(_q, frags, nfrag, seed, ticket);
        if (rc == SCCSUM_EBUSY) return false;
        detail::check(rc, "sccsum_burst_submit_mapped");
        return true;
    }
    // tx form (SCCSUM_PIPE_IPV4 queues): while a fill mode (SCCSUM_FILL_*) is
    // set, each batch generates its packets' checksums and stores them in the
    // mapped fragments themselves — at completion the mbufs are wire-ready,
    // `done` gets the values stored and the fill status bits, and submit()
    // (whose bytes are copies) throws.  0 = values only.  false: a packet is
    // staged or in flight (drain, then set again).
    bool set_fill(uint32_t mode) {
        const int rc = sccsum_burst_set_fill(_q, mode);
        if (rc == SCCSUM_EBUSY) return false;
        detail::check(rc, "sccsum_burst_set_fill");
        return true;
    }
    bool poll() {
        int did = 0;
        detail::check(sccsum_burst_poll(_q, &did), "sccsum_burst_poll");
        return did != 0;
    }
    void drain() { detail::check(sccsum_burst_drain(_q), "sccsum_burst_drain"); }
};

// Resident engine (<sccsum.h> sccsum_engine_*): one grid kept on the GPU
// while the shards stream steps into it, as the reactor keeps polling its
// queues (reactor.cc:3543-3550); each step is up to 4 batches, computed
// exactly as the one-launch calls compute them.  A run takes any number of
// steps (their descriptors cycle through a ring of ring_slots slots), and
// any number of threads may submit into it and wait — the shards that share
// the GPU; start / stop / the destructor are the owner's.  Frames engines may
// take in-place fills (fill = true).  One engine runs per device at a time:
// try_start() is false while another engine of the process runs there.
//   resident_engine eng(gpu, SCCSUM_PIPE_IPV4, /*ring_slots=*/1024, /*in flight=*/8, /*fill=*/true);
//   eng.start(stream);
//   sccsum_batch tx = {...}, rx = {...};
//   uint64_t a = eng.submit_fill(&tx, 1, SCCSUM_FILL_IP | SCCSUM_FILL_L4);   // from any shard
//   uint64_t b = eng.submit(&rx, 1);
//   eng.wait(b); eng.wait(a); eng.stop();
class resident_engine {
    detail::handle<sccsum_engine, sccsum_engine_destroy> _e;

public:
    resident_engine(int device, int mode, uint32_t ring_slots, uint32_t max_in_flight, bool fill = false) {
        detail::check(sccsum_engine_create(device, mode | (fill ? SCCSUM_ENGINE_FILL : 0), ring_slots, max_in_flight,
                                           _e.out()),
                      "sccsum_engine_create");
    }
    // every limit (ring, in flight, idle and dependency limits; 0 fields = defaults)
    resident_engine(int device, int mode, const sccsum_engine_opts& opts, bool fill = false) {
        detail::check(sccsum_engine_create_opts(device, mode | (fill ? SCCSUM_ENGINE_FILL : 0), &opts, _e.out()),
                      "sccsum_engine_create_opts");
    }
    // destroy now, reporting a run that left a published step undone (the destructor cannot)
    void close() { _e.close("sccsum_engine_destroy"); }

    // launch the grid on `stream` (the calling thread's current device, the engine's)
    void start(void* stream) { detail::check(sccsum_engine_start(_e.get(), stream), "sccsum_engine_start"); }
    // false: another engine of this process runs on the device (SCCSUM_EBUSY)
    bool try_start(void* stream) {
        const int rc = sccsum_engine_start(_e.get(), stream);
        if (rc == SCCSUM_EBUSY) return false;
        detail::check(rc, "sccsum_engine_start");
        return true;
    }
    // max_len: the longest packet, if known (sizes the step's tiles; 0 = from bytes_len / n)
    uint64_t submit(const sccsum_batch* batches, uint32_t nbatch, uint64_t timeout_ns = 1'000'000'000,
                    uint32_t max_len = 0) {
        uint64_t step = 0;
        detail::check(sccsum_engine_submit(_e.get(), batches, nbatch, max_len, timeout_ns, &step),
                      "sccsum_engine_submit");
        return step;
    }
    // in-place fill of every batch (d_out: the values, required); the step returned is done once
    // the frames hold their checksums
    uint64_t submit_fill(const sccsum_batch* batches, uint32_t nbatch, uint32_t mode,
                         uint64_t timeout_ns = 1'000'000'000, uint32_t max_len = 0) {
        uint64_t step = 0;
        detail::check(sccsum_engine_submit_fill(_e.get(), batches, nbatch, max_len, mode, timeout_ns, &step),
                      "sccsum_engine_submit_fill");
        return step;
    }
    void wait(uint64_t step, uint64_t timeout_ns = 1'000'000'000) {
        detail::check(sccsum_engine_wait(_e.get(), step, timeout_ns), "sccsum_engine_wait");
    }
    void stop() { detail::check(sccsum_engine_stop(_e.get()), "sccsum_engine_stop"); }
};

// Rx steering (<sccsum.h> sccsum_steer_*): device::hash2cpu / forward_dst
// (net.hh:287-305) for a whole rx batch, and the batch's packet indices
// grouped by destination shard in arrival order — what dispatch_packet's
// forward() (net.cc:330-344) builds one packet at a time.  Immutable after
// construction: every shard of the GPU may run the same object on its own
// stream.
//   uint8_t reta[128];
//   rx_steering::build_reta(cpus, weights, ncpu, reta);          // qp::build_sw_reta, net.cc:214-231
//   sccsum_steer_map map = {ncpu, 1, 0, 0, nullptr, reta, nullptr};
//   rx_steering steer(gpu, map);
//   engine.ipv4_frames_rss(batch, key, key_len, SCCSUM_RSS_DISPATCH, nullptr, d_status, d_hash, stream);
//   steer.run(SCCSUM_STEER_HASH2CPU, 0, d_hash, d_status, SCCSUM_ST_OK, SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE,
//             batch.n, d_cpu, d_order, d_first, d_ws, stream);   // shard c: d_order[d_first[c] .. d_first[c+1])
class rx_steering {
    detail::handle<sccsum_steer, sccsum_steer_destroy> _s;

public:
    // validates every table entry and copies the tables (host memory) to `device`
    rx_steering(int device, const sccsum_steer_map& map) {
        detail::check(sccsum_steer_create(device, &map, _s.out()), "sccsum_steer_create");
    }
    void close() { _s.close("sccsum_steer_destroy"); }

    // bytes of 16-byte aligned device scratch a run over n packets needs
    uint64_t workspace(uint64_t n) const noexcept { return sccsum_steer_workspace(_s.get(), n); }

    // mode SCCSUM_STEER_DISPATCH (forward_dst(src_cpu, hash)) or SCCSUM_STEER_HASH2CPU; a packet whose
    // status lacks a `need` bit or has a `reject` bit is dropped (d_status null: none, masks 0).
    // d_cpu[n] (0xFF = dropped) and d_order[n] may be null; d_first has ncpu + 2 entries.
    void run(int mode, uint32_t src_cpu, const uint32_t* d_hash, const uint8_t* d_status, uint32_t need,
             uint32_t reject, uint64_t n, uint8_t* d_cpu, uint32_t* d_order, uint32_t* d_first, void* d_workspace,
             void* stream) const {
        detail::check(sccsum_steer_run(_s.get(), mode, src_cpu, d_hash, d_status, need, reject, n, d_cpu, d_order,
                                       d_first, d_workspace, stream),
                      "sccsum_steer_run");
    }

    // qp::build_sw_reta (net.cc:214-231): cpus strictly ascending, as the reference's std::map iterates
    static void build_reta(const uint32_t* cpus, const float* weights, uint32_t n, uint8_t (&reta)[128]) {
        detail::check(sccsum_steer_build_reta(cpus, weights, n, reta), "sccsum_steer_build_reta");
    }

    // one hash through the map on the host: device::hash2cpu (SCCSUM_STEER_HASH2CPU) / forward_dst
    static uint32_t dest(const sccsum_steer_map& map, int mode, uint32_t src_cpu, uint32_t hash) {
        const uint32_t d = sccsum_steer_dest(&map, mode, src_cpu, hash);
        if (d == UINT32_MAX) detail::check(SCCSUM_EINVAL, "sccsum_steer_dest");
        return d;
    }
};

// Rx reassembly (<sccsum.h> sccsum_ipv4_frag_records / sccsum_ipv4_reasm): the
// reassembly branch of ipv4::handle_received_packet (ip.cc:164-220) with
// frag::merge / is_complete (ip.cc:412-437) and packet_merger::merge
// (packet-util.hh:45-151) for a batch's fragments.  No payload byte moves: a
// complete datagram is a fragment list for spans_desc (its L4 verify) and
// sccsum_gather, its hash goes to rx_steering::run.  Keys whose outcome depends
// on arrival order (overlaps, duplicates) come back in the host bucket, for the
// stack's own merger; frag_timeout / frag_limit_mem stay with the stack (the
// records' tag).  Stateless: any thread, any stream of the data's device.
//   rx_reassembler rx(host_address);
//   engine.ipv4_frames_rss(batch, key, key_len, SCCSUM_RSS_DISPATCH, nullptr, d_status, d_hash, stream);
//   rx.records(batch, d_status, now, d_rec + carried, d_count, d_ws, stream);   // behind the carried records
//   rx.run(d_rec, carried + count, max_bytes, key, key_len, out, d_ws, stream);
//   engine.spans_desc(out.d_desc, out.d_dgram_first, out.d_dgram_off, out.d_dgram_len, datagrams, 65535,
//                     nullptr, out.d_dgram_seed, d_l4, d_l4_status, stream);      // 0 = L4 verifies
//   steer.run(SCCSUM_STEER_HASH2CPU, 0, out.d_dgram_hash, ...);                  // out.d_pending: the next carry
class rx_reassembler {
    uint32_t _host;

public:
    // host_address: ipv4::_host_address (host order); 0 accepts every destination
    explicit rx_reassembler(uint32_t host_address) : _host(host_address) {}

    uint32_t host_address() const noexcept { return _host; }

    // bytes of 16-byte aligned device scratch records() over n frames / run() over m records needs
    static uint64_t workspace(uint64_t m) noexcept { return sccsum_ipv4_reasm_workspace(m); }

    // the 32-bit mix of a key that run() groups by
    static uint32_t key_mix(uint32_t src_host, uint32_t dst_host, uint16_t id, uint8_t proto) noexcept {
        return sccsum_reasm_key_mix(src_host, dst_host, id, proto);
    }

    // One record per fragment of the batch that ip.cc:121-162 lets through, in arrival order, given
    // the d_status the frames call wrote; *d_count = their number.  need / reject as in rx_steering.
    void records(const device_packet_batch& b, const uint8_t* d_status, uint32_t tag, sccsum_frag_rec* d_rec,
                 uint32_t* d_count, void* d_workspace, void* stream,
                 uint32_t need = SCCSUM_ST_OK | SCCSUM_ST_IPFRAG,
                 uint32_t reject = SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE) const {
        detail::check(sccsum_ipv4_frag_records(b.bytes, b.bytes_len, b.off, b.len, d_status, need, reject, b.n, _host,
                                               tag, d_rec, d_count, d_workspace, stream),
                      "sccsum_ipv4_frag_records");
    }

    // m records in arrival order, the pending ones of the last run first.  key may be null (then
    // out.d_dgram_hash must be).  Capacity is a prefix rule: what does not fit stays pending.
    void run(const sccsum_frag_rec* d_rec, uint64_t m, uint64_t max_out_bytes, const uint8_t* key, size_t key_len,
             const sccsum_reasm_out& out, void* d_workspace, void* stream) const {
        detail::check(sccsum_ipv4_reasm(d_rec, m, max_out_bytes, key, static_cast<uint32_t>(key_len), &out, d_workspace,
                                        stream),
                      "sccsum_ipv4_reasm");
    }
};

// Tx send (<sccsum.h> sccsum_ipv4_send*): ipv4::send (ip.cc:244-299) for a
// batch of L4 datagrams that lie in device memory — every frame's IPv4 header
// and, for a datagram past the MTU (needs_frag, ip.cc:100-111), the cut into
// fragments.  Like the reference's p.share(offset, can_send) + prepend, no
// payload byte moves: a frame is a 20-byte header and two fragment records, so
// the outputs feed ipv4_frames_desc / ipv4_fill_desc / a burst queue's mapped
// form as they stand, and sccsum_gather packs them.  Stateless: any thread,
// any stream of the data's device.
//   tx_sender tx(host_address, hw.mtu, hw.tx_tso ? SCCSUM_SEND_TSO : 0);
//   engine.sum_spans(l4, d_seeds, d_l4sum, nullptr, stream);          // pseudo-header seeds, fields zero
//   tx.run(l4, d_dst, d_proto, d_id, d_l4sum, max_frames, max_bytes, out, tx.workspace(l4.n) sized d_ws, stream);
//   engine.ipv4_fill_desc(out.desc, out.first, out.out_off, out.out_len, frames, mtu, SCCSUM_FILL_IP, ...);
class tx_sender {
    sccsum_send_opts _opts;

public:
    // what a run writes (device arrays; sizes in <sccsum.h>, "Tx send")
    struct outputs {
        uint8_t* hdr = nullptr;               // 20 * max_frames bytes
        sccsum_gather_desc* desc = nullptr;   // 2 * max_frames records
        uint32_t* first = nullptr;            // max_frames + 1
        uint64_t* out_off = nullptr;          // max_frames
        uint32_t* out_len = nullptr;          // max_frames
        uint32_t* dgram_first = nullptr;      // n + 1
        uint8_t* status = nullptr;            // n
        uint64_t* total = nullptr;            // 3: frames needed, bytes needed, datagrams emitted
    };
    struct plan_result {
        uint32_t frames;     // 0: the datagram is refused (longer than 65515 bytes)
        uint64_t out_bytes;  // its bytes in the packed layout
    };

    // src_host: ipv4::_host_address (host order); mtu: hw_features().mtu; flags: SCCSUM_SEND_*
    // (SCCSUM_SEND_L4 is added by run() when it is given the L4 values)
    tx_sender(uint32_t src_host, uint32_t mtu, uint32_t flags = 0) : _opts{src_host, mtu, flags} {}

    const sccsum_send_opts& opts() const noexcept { return _opts; }

    // host arithmetic for one datagram; throws on an MTU outside 68..65535 or unknown flags
    static plan_result plan(const sccsum_send_opts& opts, uint32_t l4_len, uint8_t proto) {
        plan_result r{0, 0};
        detail::check(sccsum_ipv4_send_plan(&opts, l4_len, proto, &r.frames, &r.out_bytes), "sccsum_ipv4_send_plan");
        return r;
    }
    plan_result plan(uint32_t l4_len, uint8_t proto) const { return plan(_opts, l4_len, proto); }

    // bytes of 16-byte aligned device scratch a run over n datagrams needs
    static uint64_t workspace(uint64_t n) noexcept { return sccsum_ipv4_send_workspace(n); }

    // l4: the datagrams (bytes is written only through d_l4sum's values); d_dst host-order
    // addresses; d_id may be null (id 0); d_l4sum null, or the values to store in the UDP / TCP
    // checksum fields before the cut.  Capacity is a prefix rule (out.total reports the need).
    void run(const device_packet_batch& l4, const uint32_t* d_dst, const uint8_t* d_proto, const uint16_t* d_id,
             const uint16_t* d_l4sum, uint64_t max_frames, uint64_t max_out_bytes, const outputs& out,
             void* d_workspace, void* stream) const {
        sccsum_send_opts o = _opts;
        if (d_l4sum) o.flags |= SCCSUM_SEND_L4;
        detail::check(sccsum_ipv4_send(&o, const_cast<void*>(l4.bytes), l4.bytes_len, l4.off, l4.len, d_dst, d_proto,
                                       d_id, d_l4sum, l4.n, max_frames, max_out_bytes, out.hdr, out.desc, out.first,
                                       out.out_off, out.out_len, out.dgram_first, out.status, out.total, d_workspace,
                                       stream),
                      "sccsum_ipv4_send");
    }
};

// ARP table (<sccsum.h> sccsum_arp_table_*): an immutable device copy of what
// arp_for<ipv4>::_table holds (arp.hh:153, 214-216, 247-248), for eth_rx::learn
// and eth_tx::run.  A changed table is a new object; the old one is destroyed
// once its stream is synchronised.  A MAC is the six wire bytes as a
// big-endian number in a uint64_t.
//   sccsum_arp_entry e[] = {{0xFFFFFFFFu, 0, 0xFFFFFFFFFFFFull}, {peer_ip, 0, peer_mac}};
//   arp_table arp(gpu, e, 2);
class arp_table {
    detail::handle<sccsum_arp_table, sccsum_arp_table_destroy> _t;

public:
    // entries: host memory, a later entry for the same ip wins; n <= 2^20
    arp_table(int device, const sccsum_arp_entry* entries, uint32_t n) {
        detail::check(sccsum_arp_table_create(device, entries, n, _t.out()), "sccsum_arp_table_create");
    }
    // no device copy: lookup() alone
    arp_table(const sccsum_arp_entry* entries, uint32_t n) {
        detail::check(sccsum_arp_table_create_host(entries, n, _t.out()), "sccsum_arp_table_create_host");
    }

    const sccsum_arp_table* get() const noexcept { return _t.get(); }
    uint32_t bits() const noexcept { return sccsum_arp_table_bits(get()); }

    // host arithmetic: true and *mac on a hit
    bool lookup(uint32_t ip, uint64_t* mac) const noexcept { return sccsum_arp_table_lookup(get(), ip, mac) != 0; }

    // a key's home slot in a table of 2^bits slots
    static uint32_t slot(uint32_t ip, uint32_t bits) noexcept { return sccsum_arp_table_slot(ip, bits); }
};

// Link-layer rx (<sccsum.h> sccsum_eth_rx / sccsum_arp_learn_records):
// interface::dispatch_packet (net.cc:324-357) for a batch of wire frames — the
// frames grouped by registered eth_proto with the 14-byte trim, so an IPv4
// bucket is a frames batch for ipv4_frames* as it stands — and the learn
// candidates of ip.cc:147-149 among an IPv4 bucket.  Stateless: any thread,
// any stream of the data's device.
//   eth_rx rx({0x0800, 0x0806});
//   rx.run(wire, out, d_ws, stream);                  // out.first copied back: the bucket bounds
//   device_packet_batch ip{wire.bytes, wire.bytes_len, out.l3_off + first[0], out.l3_len + first[0], count, 0};
//   engine.ipv4_frames(ip, nullptr, d_status, stream);
//   rx.learn(ip, d_status, out.src_mac + first[0], host, netmask, &arp, d_rec, d_count, d_ws, stream);
class eth_rx {
    uint16_t _protos[SCCSUM_ETH_MAX_PROTOS] = {};
    uint32_t _k = 0;

public:
    // what run() writes (device arrays; sizes in <sccsum.h>, "Link layer")
    struct outputs {
        uint8_t* cls = nullptr;        // n, optional
        uint32_t* first = nullptr;     // protos + 2
        uint32_t* order = nullptr;     // n
        uint64_t* l3_off = nullptr;    // n
        uint32_t* l3_len = nullptr;    // n
        uint64_t* src_mac = nullptr;   // n
    };

    // the registered eth_proto values (host order), 1..8 distinct ones: bucket k is protos[k]
    eth_rx(std::initializer_list<uint16_t> protos) {
        if (protos.size() < 1 || protos.size() > SCCSUM_ETH_MAX_PROTOS) detail::check(SCCSUM_EINVAL, "eth_rx");
        for (uint16_t p : protos) _protos[_k++] = p;
    }

    uint32_t protos() const noexcept { return _k; }

    static uint64_t workspace(uint64_t n) noexcept { return sccsum_eth_rx_workspace(n); }
    static uint64_t learn_workspace(uint64_t n) noexcept { return sccsum_arp_learn_workspace(n); }

    void run(const device_packet_batch& wire, const outputs& out, void* d_workspace, void* stream) const {
        detail::check(sccsum_eth_rx(wire.bytes, wire.bytes_len, wire.off, wire.len, wire.n, _protos, _k, out.cls,
                                    out.first, out.order, out.l3_off, out.l3_len, out.src_mac, d_workspace, stream),
                      "sccsum_eth_rx");
    }

    // ip: an IPv4 bucket; d_status what the frames call wrote for it; d_src_mac the bucket's slice.
    // table may be null (maps nothing).  d_rec has room for ip.n records; *d_count = their number.
    static void learn(const device_packet_batch& ip, const uint8_t* d_status, const uint64_t* d_src_mac, uint32_t host,
                      uint32_t netmask, const arp_table* table, sccsum_arp_rec* d_rec, uint32_t* d_count,
                      void* d_workspace, void* stream, uint32_t need = SCCSUM_ST_OK,
                      uint32_t reject = SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE) {
        detail::check(sccsum_arp_learn_records(ip.bytes, ip.bytes_len, ip.off, ip.len, d_status, need, reject,
                                               d_src_mac, ip.n, host, netmask, table ? table->get() : nullptr, d_rec,
                                               d_count, d_workspace, stream),
                      "sccsum_arp_learn_records");
    }
};

// Link-layer tx (<sccsum.h> sccsum_eth_send): ipv4::get_l2_dst_address
// (ip.cc:231-242) per datagram and the Ethernet header the interface's packet
// provider prepends (net.cc:266-284), on tx_sender's fragment lists after
// their checksum fills: one more descriptor in front of every frame, no
// payload byte moves.  Datagrams whose next hop has no ARP entry are listed
// for the host's ARP queries instead.  Stateless.
//   eth_tx tx({hw_address, host, netmask, gw, 0x0800});
//   tx.run(arp, d_dst, send_out.dgram_first, n, send_out.desc, send_out.first, send_out.out_off, send_out.out_len,
//          frames, max_bytes, out, d_ws, stream);
class eth_tx {
    sccsum_eth_opts _opts;

public:
    // what run() writes (device arrays; sizes in <sccsum.h>, "Link layer")
    struct outputs {
        uint8_t* eth = nullptr;                       // 14 * frames bytes
        sccsum_gather_desc* desc = nullptr;           // descriptors + frames records
        uint32_t* first = nullptr;                    // frames + 1
        uint64_t* out_off = nullptr;                  // frames
        uint32_t* out_len = nullptr;                  // frames
        uint32_t* frame_src = nullptr;                // frames
        uint8_t* status = nullptr;                    // n
        sccsum_eth_unresolved* unresolved = nullptr;  // n
        uint64_t* total = nullptr;                    // 6
    };

    explicit eth_tx(const sccsum_eth_opts& opts) : _opts(opts) {}

    const sccsum_eth_opts& opts() const noexcept { return _opts; }

    static uint64_t workspace(uint64_t n) noexcept { return sccsum_eth_send_workspace(n); }

    // d_dgram_first may be null: one frame per datagram (frames == n)
    void run(const arp_table& table, const uint32_t* d_dst, const uint32_t* d_dgram_first, uint64_t n,
             const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off, const uint32_t* d_len,
             uint64_t frames, uint64_t max_out_bytes, const outputs& out, void* d_workspace, void* stream) const {
        detail::check(sccsum_eth_send(&_opts, table.get(), d_dst, d_dgram_first, n, d_desc, d_first, d_off, d_len,
                                      frames, max_out_bytes, out.eth, out.desc, out.first, out.out_off, out.out_len,
                                      out.frame_src, out.status, out.unresolved, out.total, d_workspace, stream),
                      "sccsum_eth_send");
    }
};

// UDP port table (<sccsum.h> sccsum_udp_ports_*): an immutable device copy of
// what ipv4_udp::_channels maps (udp.cc:168-169, 235-236): channel k is
// ports[k].  A changed set of channels is a new object; the old one is
// destroyed once its stream is synchronised.
//   const uint16_t bound[] = {53, 10000};
//   udp_ports ports(gpu, bound, 2);
class udp_ports {
    detail::handle<sccsum_udp_ports, sccsum_udp_ports_destroy> _t;

public:
    // ports: host memory, distinct, host order; channels <= SCCSUM_UDP_MAX_CHANNELS
    udp_ports(int device, const uint16_t* ports, uint32_t channels) {
        detail::check(sccsum_udp_ports_create(device, ports, channels, _t.out()), "sccsum_udp_ports_create");
    }
    // no device copy: lookup() alone
    udp_ports(const uint16_t* ports, uint32_t channels) {
        detail::check(sccsum_udp_ports_create_host(ports, channels, _t.out()), "sccsum_udp_ports_create_host");
    }

    const sccsum_udp_ports* get() const noexcept { return _t.get(); }
    uint32_t channels() const noexcept { return sccsum_udp_ports_channels(get()); }

    // host arithmetic: the channel bound to port, or -1
    int lookup(uint16_t port) const noexcept { return sccsum_udp_ports_lookup(get(), port); }
};

// UDP rx (<sccsum.h> sccsum_udp_rx / sccsum_udp_rx_reasm): the end of
// ipv4::handle_received_packet (ip.cc:159-162, 222-227) and ipv4_udp::received
// (udp.cc:45-53, 164-173) for a batch — the non-fragment frames of an IPv4
// bucket, or the datagrams rx_reassembler delivered, grouped by channel with
// both headers trimmed; no byte moves.  The reference verifies no UDP checksum
// on rx; need = SCCSUM_ST_OK | SCCSUM_ST_L4_OK does.  Stateless apart from the
// addresses it was made with.
//   udp_rx rx(ports, host);
//   rx.run(ip, d_status, nullptr, ip.n, out, d_ws, stream);       // out.first copied back: the channel bounds
//   uint64_t q = udp_rx::taken(first[k + 1] - first[k], room);    // what the channel's queue accepts
class udp_rx {
    const udp_ports& _ports;
    uint32_t _host;

public:
    // what run() / run_reassembled() write (device arrays; sizes in <sccsum.h>, "UDP layer")
    struct outputs {
        uint8_t* cls = nullptr;        // n, optional
        uint32_t* first = nullptr;     // channels + 2
        uint32_t* order = nullptr;     // n
        uint64_t* pay_off = nullptr;   // n (run() only)
        uint32_t* pay_len = nullptr;   // n
        uint32_t* src = nullptr;       // n
        uint16_t* sport = nullptr;     // n
    };

    // what run_reassembled() reads of rx_reassembler's output
    struct datagrams {
        const sccsum_gather_desc* desc = nullptr;
        const uint32_t* dgram_first = nullptr;  // m + 1
        const uint64_t* dgram_off = nullptr;    // m
        const uint32_t* dgram_len = nullptr;    // m
        const uint32_t* dgram_head = nullptr;   // m
        uint64_t m = 0;
        const sccsum_frag_rec* rec = nullptr;   // the records reassembly took
        uint64_t nrec = 0;
    };

    // host_address 0 accepts any destination; `ports` must outlive the object
    udp_rx(const udp_ports& ports, uint32_t host_address) : _ports(ports), _host(host_address) {}

    uint32_t host_address() const noexcept { return _host; }

    static uint64_t workspace(uint64_t n) noexcept { return sccsum_udp_rx_workspace(n); }
    static uint64_t reassembled_workspace(uint64_t m) noexcept { return sccsum_udp_rx_reasm_workspace(m); }

    // _queue.push with `room` free slots keeps the first taken() datagrams of a channel's bucket (queue.hh:184-192)
    static uint64_t taken(uint64_t count, uint64_t room) noexcept { return count < room ? count : room; }

    // ip: an IPv4 bucket; d_status what the frames call wrote for it; d_index (may be null: frame j is
    // batch frame j) the n batch frame indices of this call, e.g. a shard's slice of rx_steering's order
    void run(const device_packet_batch& ip, const uint8_t* d_status, const uint32_t* d_index, uint64_t n,
             const outputs& out, void* d_workspace, void* stream, uint32_t need = SCCSUM_ST_OK,
             uint32_t reject = SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE | SCCSUM_ST_IPFRAG) const {
        detail::check(sccsum_udp_rx(ip.bytes, ip.bytes_len, ip.off, ip.len, ip.n, d_status, need, reject, _host,
                                    _ports.get(), d_index, n, out.cls, out.first, out.order, out.pay_off, out.pay_len,
                                    out.src, out.sport, d_workspace, stream),
                      "sccsum_udp_rx");
    }

    // d_l4_status: what spans_desc wrote for the datagrams' L4 verify, or null (the masks then 0)
    void run_reassembled(const datagrams& in, const uint8_t* d_l4_status, const outputs& out, void* d_workspace,
                         void* stream, uint32_t need = 0, uint32_t reject = 0) const {
        detail::check(sccsum_udp_rx_reasm(in.desc, in.dgram_first, in.dgram_off, in.dgram_len, in.dgram_head, in.m,
                                          in.rec, in.nrec, d_l4_status, need, reject, _host, _ports.get(), out.cls,
                                          out.first, out.order, out.pay_len, out.src, out.sport, d_workspace, stream),
                      "sccsum_udp_rx_reasm");
    }
};

// UDP tx (<sccsum.h> sccsum_udp_send): ipv4_udp::send's header (udp.cc:175-197)
// written into the 8 bytes of headroom in front of every payload, and the
// spans and seeds of the checksum pass whose results tx_sender stores
// (SCCSUM_SEND_L4); no payload byte moves.  Stateless.
//   udp_tx tx({host, 1500, 0});
//   tx.run(d_bytes, bytes_len, d_off, d_len, n, d_dst, d_dport, d_sport, out, stream);
//   engine.sum_spans({d_bytes, bytes_len, out.l4_off, out.sum_len, n, 0}, out.seed, d_l4sum, ...);
class udp_tx {
    sccsum_udp_opts _opts;

public:
    // what run() writes (device arrays of n entries; <sccsum.h>, "UDP layer")
    struct outputs {
        uint64_t* l4_off = nullptr;
        uint32_t* l4_len = nullptr;
        uint32_t* sum_len = nullptr;
        uint32_t* seed = nullptr;
        uint8_t* proto = nullptr;       // optional
        uint8_t* needs_csum = nullptr;
        uint8_t* status = nullptr;
    };

    explicit udp_tx(const sccsum_udp_opts& opts) : _opts(opts) {}

    const sccsum_udp_opts& opts() const noexcept { return _opts; }

    // d_bytes is written: 8 bytes in front of every accepted payload
    void run(void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len, uint64_t n,
             const uint32_t* d_dst, const uint16_t* d_dport, const uint16_t* d_sport, const outputs& out,
             void* stream) const {
        detail::check(sccsum_udp_send(&_opts, d_bytes, bytes_len, d_off, d_len, d_dst, d_dport, d_sport, n, out.l4_off,
                                      out.l4_len, out.sum_len, out.seed, out.proto, out.needs_csum, out.status, stream),
                      "sccsum_udp_send");
    }
};

// TCP connection table (<sccsum.h> sccsum_tcp_conns_*): an immutable device
// copy of what tcp::_tcbs maps (tcp.hh:885-886) and of the ports of
// tcp::_listening: connection c is conns[c], whatever its state.  A changed
// set of connections is a new object; the old one is destroyed once its
// stream is synchronised.
//   const sccsum_tcp_conn c[] = {{me, peer, 80, 40000}};
//   const uint16_t listening[] = {80};
//   tcp_conns conns(gpu, c, 1, listening, 1);
class tcp_conns {
    detail::handle<sccsum_tcp_conns, sccsum_tcp_conns_destroy> _t;

public:
    // conns, listen: host memory, distinct, host order; nconns <= SCCSUM_TCP_MAX_CONNS, nlisten <= 65536
    tcp_conns(int device, const sccsum_tcp_conn* conns, uint32_t nconns, const uint16_t* listen, uint32_t nlisten) {
        detail::check(sccsum_tcp_conns_create(device, conns, nconns, listen, nlisten, _t.out()),
                      "sccsum_tcp_conns_create");
    }
    // no device copy: lookup() and listening() alone
    tcp_conns(const sccsum_tcp_conn* conns, uint32_t nconns, const uint16_t* listen, uint32_t nlisten) {
        detail::check(sccsum_tcp_conns_create_host(conns, nconns, listen, nlisten, _t.out()),
                      "sccsum_tcp_conns_create_host");
    }

    const sccsum_tcp_conns* get() const noexcept { return _t.get(); }
    uint32_t count() const noexcept { return sccsum_tcp_conns_count(get()); }
    uint32_t bits() const noexcept { return sccsum_tcp_conns_bits(get()); }

    // host arithmetic: the connection of a connid, or -1; is the port listening
    int64_t lookup(const sccsum_tcp_conn& id) const noexcept {
        return sccsum_tcp_conns_lookup(get(), id.local_ip, id.foreign_ip, id.local_port, id.foreign_port);
    }
    bool listening(uint16_t port) const noexcept { return sccsum_tcp_conns_listening(get(), port) != 0; }
    // the home slot of a connid in a table of 2^bits slots
    static uint32_t slot(const sccsum_tcp_conn& id, uint32_t bits) noexcept {
        return sccsum_tcp_conns_slot(id.local_ip, id.foreign_ip, id.local_port, id.foreign_port, bits);
    }
};

// TCP rx (<sccsum.h> sccsum_tcp_rx): the stateless part of tcp::received
// (tcp.hh:865-942) for the non-fragment frames of an IPv4 bucket — the header
// parsed, the connid looked up, then the listening ports, then the RST of
// respond_with_reset (tcp.hh:981-1023) — ending in segments grouped per
// connection in arrival order; no byte moves.  The state machine stays the
// caller's, per connection.  Stateless apart from what it was made with.
//   tcp_rx rx(conns, host);
//   rx.run(ip, d_status, nullptr, ip.n, out, d_ws, stream);      // out.first, out.total copied back
//   uint64_t q = tcp_rx::taken(total[1], queue_space);           // the answers send_packet_without_tcb accepts
class tcp_rx {
    const tcp_conns& _conns;
    uint32_t _host;
    uint32_t _flags;

public:
    // what run() writes (device arrays; sizes in <sccsum.h>, "TCP layer")
    struct outputs {
        uint8_t* cls = nullptr;          // n, optional
        uint32_t* first = nullptr;       // 5
        uint32_t* order = nullptr;       // n
        sccsum_tcp_seg* seg = nullptr;   // n
        uint32_t* src = nullptr;         // n
        uint32_t* run_conn = nullptr;    // min(n, count) + 1
        uint32_t* run_first = nullptr;   // min(n, count) + 1
        void* rst = nullptr;             // 20 n bytes
        uint32_t* rst_dst = nullptr;     // n
        uint64_t* total = nullptr;       // 4: R, resets
    };

    // host_address 0 accepts any destination; flags: SCCSUM_TCP_CSUM_OFFLOAD for the answers; `conns` must outlive the object
    tcp_rx(const tcp_conns& conns, uint32_t host_address, uint32_t flags = 0)
        : _conns(conns), _host(host_address), _flags(flags) {}

    uint32_t host_address() const noexcept { return _host; }

    uint64_t workspace(uint64_t n) const noexcept { return sccsum_tcp_rx_workspace(n, _conns.count()); }

    // send_packet_without_tcb with `space` bytes of _queue_space keeps the first taken() answers (tcp.hh:946-953)
    static uint64_t taken(uint64_t resets, uint64_t space) noexcept { return resets < space / 20 ? resets : space / 20; }

    // ip: an IPv4 bucket; d_status what the frames call wrote for it; d_index (may be null: frame j is
    // batch frame j) the n batch frame indices of this call, e.g. a shard's slice of rx_steering's order
    void run(const device_packet_batch& ip, const uint8_t* d_status, const uint32_t* d_index, uint64_t n,
             const outputs& out, void* d_workspace, void* stream, uint32_t need = SCCSUM_ST_OK | SCCSUM_ST_L4_OK,
             uint32_t reject = SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE | SCCSUM_ST_IPFRAG) const {
        detail::check(sccsum_tcp_rx(ip.bytes, ip.bytes_len, ip.off, ip.len, ip.n, d_status, need, reject, _host,
                                    _conns.get(), d_index, n, _flags, out.cls, out.first, out.order, out.seg, out.src,
                                    out.run_conn, out.run_first, out.rst, out.rst_dst, out.total, d_workspace, stream),
                      "sccsum_tcp_rx");
    }
};

// TCP rx, the data (<sccsum.h> sccsum_tcp_rx_data): header prediction for a
// batch.  The leading stretch of every run of tcp_rx's bucket 0 that is
// acceptable, exactly at RCV.NXT, carries text, no control flag besides ACK /
// PSH and acknowledges nothing new — step 4.7 of input_handle_other_state
// (tcp.hh:1497-1521) and nothing else — becomes one run record and one gather
// descriptor per segment; the rest of a run is the tcb's to walk, from the
// state in the record.  No byte moves.
//   tcp_rx_data data(conns.count());
//   data.run(ip.bytes, rx_out, n, d_rcv, max_bytes, out, d_ws, stream);   // rx_out: what tcp_rx::run wrote
//   sccsum_gather(out.desc, total[0], d_stream_buf, stream);             // run r's bytes at [dst_off, + bytes)
class tcp_rx_data {
    uint32_t _nconns;

public:
    // what run() writes (device arrays; <sccsum.h>, "TCP receive fast path")
    struct outputs {
        sccsum_tcp_rcv_run* run = nullptr;   // min(n, nconns) + 1
        sccsum_gather_desc* desc = nullptr;  // n
        uint64_t* total = nullptr;           // 4: taken, bytes as emitted; the bytes needed
    };

    // nconns: the entries of d_rcv, the table's count()
    explicit tcp_rx_data(uint32_t nconns) : _nconns(nconns) {}

    uint32_t nconns() const noexcept { return _nconns; }

    uint64_t workspace(uint64_t n) const noexcept { return sccsum_tcp_rx_data_workspace(n, _nconns); }

    // d_bytes: the frames' buffer (never read); rx, n: tcp_rx::run's outputs as they stand on the device and
    // its n; d_rcv: one sccsum_tcp_rcv per connection, 16-byte aligned; max_bytes <= 2^32 - 1
    void run(const void* d_bytes, const tcp_rx::outputs& rx, uint64_t n, const sccsum_tcp_rcv* d_rcv,
             uint64_t max_bytes, const outputs& out, void* d_workspace, void* stream) const {
        detail::check(sccsum_tcp_rx_data(d_bytes, rx.seg, rx.first, rx.run_conn, rx.run_first, rx.total, n, d_rcv,
                                         _nconns, max_bytes, out.run, out.desc, out.total, d_workspace, stream),
                      "sccsum_tcp_rx_data");
    }
};

// TCP tx (<sccsum.h> sccsum_tcp_send): tcb::output_one's header (tcp.hh:1620-1698)
// written into the hdr_len bytes of headroom in front of every payload, the
// caller's options behind it, and the spans and seeds of the checksum pass
// whose results tx_sender stores (SCCSUM_SEND_L4); no payload byte moves.
//   tcp_tx tx({host, 1500, 0});
//   tx.run(d_bytes, bytes_len, d_off, d_len, d_out, n, out, stream);
//   engine.sum_spans({d_bytes, bytes_len, out.l4_off, out.sum_len, n, 0}, out.seed, d_l4sum, ...);
class tcp_tx {
    sccsum_tcp_opts _opts;

public:
    // what run() writes (device arrays of n entries; <sccsum.h>, "TCP layer")
    struct outputs {
        uint64_t* l4_off = nullptr;
        uint32_t* l4_len = nullptr;
        uint32_t* sum_len = nullptr;
        uint32_t* seed = nullptr;
        uint16_t* tso_seg = nullptr;
        uint8_t* proto = nullptr;       // optional
        uint8_t* needs_csum = nullptr;
        uint8_t* status = nullptr;
    };

    explicit tcp_tx(const sccsum_tcp_opts& opts) : _opts(opts) {}

    const sccsum_tcp_opts& opts() const noexcept { return _opts; }

    // d_bytes is written: the twenty fixed bytes at d_off - hdr_len of every accepted segment
    void run(void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
             const sccsum_tcp_out* d_out, uint64_t n, const outputs& out, void* stream) const {
        detail::check(sccsum_tcp_send(&_opts, d_bytes, bytes_len, d_off, d_len, d_out, n, out.l4_off, out.l4_len,
                                      out.sum_len, out.seed, out.tso_seg, out.proto, out.needs_csum, out.status,
                                      stream),
                      "sccsum_tcp_send");
    }
};

// TCP tx, the data (<sccsum.h> sccsum_tcp_tx_data): the cut tcb::get_packet's
// chain makes of every polled connection's unsent queue — can_send(),
// get_transmit_packet() and output_one's seq (tcp.hh:515-549, 1578-1606,
// 1635-1645) — for the tcbs on the straight path: one run record per
// connection, and per segment its place in a packed layout, its sccsum_tcp_out
// and its gather descriptors, as tcp_tx::run takes them.  No byte moves.
//   tcp_tx_data cut({host, 1500, 65535, 20, 0});
//   cut.run(d_snd, nconns, queues, max_segs, max_out_bytes, out, d_ws, stream);
//   sccsum_gather(out.desc, total[2], d_staging, stream);   // the _snd.data clones: the buffers are free
//   tx.run(d_staging, total[1], out.off, out.len, out.out, total[0], tx_out, stream);
class tcp_tx_data {
    sccsum_tcp_tx_opts _opts;

public:
    // the unsent queues as a CSR (device arrays): connection c's buffers are [first[c], first[c + 1])
    struct queues {
        const uint64_t* src = nullptr;    // nbuf addresses: device, or pinned / registered host memory
        const uint32_t* len = nullptr;    // nbuf
        const uint32_t* first = nullptr;  // nconns + 1
        uint64_t nbuf = 0;
    };

    // what run() writes (device arrays; <sccsum.h>, "TCP transmit fast path")
    struct outputs {
        sccsum_tcp_snd_run* run = nullptr;   // nconns
        uint64_t* off = nullptr;             // max_segs
        uint32_t* len = nullptr;             // max_segs
        sccsum_tcp_out* out = nullptr;       // max_segs
        uint32_t* seg_first = nullptr;       // max_segs + 1
        sccsum_gather_desc* desc = nullptr;  // max_segs + nbuf
        uint64_t* total = nullptr;           // 4: segments, layout bytes, descriptors emitted; the bytes needed
    };

    explicit tcp_tx_data(const sccsum_tcp_tx_opts& opts) : _opts(opts) {}

    const sccsum_tcp_tx_opts& opts() const noexcept { return _opts; }

    static uint64_t workspace(uint32_t nconns, uint64_t nbuf) noexcept {
        return sccsum_tcp_tx_data_workspace(nconns, nbuf);
    }

    // d_snd: one sccsum_tcp_snd per polled connection, 16-byte aligned; max_segs <= 2^31 - 1, max_out_bytes <= 2^32 - 1
    void run(const sccsum_tcp_snd* d_snd, uint32_t nconns, const queues& q, uint64_t max_segs, uint64_t max_out_bytes,
             const outputs& out, void* d_workspace, void* stream) const {
        detail::check(sccsum_tcp_tx_data(&_opts, d_snd, nconns, q.src, q.len, q.first, q.nbuf, max_segs, max_out_bytes,
                                         out.run, out.off, out.len, out.out, out.seg_first, out.desc, out.total,
                                         d_workspace, stream),
                      "sccsum_tcp_tx_data");
    }
};

// TCP rx, the ACKs (<sccsum.h> sccsum_tcp_rx_acks): the sender half of header
// prediction for a batch.  The leading stretch of every run of tcp_rx's bucket
// 0 that is pure ACKs advancing SND.UNA — the advancing-ACK branch of
// input_handle_other_state (tcp.hh:1336-1400) with data_segment_acked,
// update_rto, update_cwnd and the window update, and nothing else — becomes one
// run record holding all the host applies to the tcb; the rest of a run is the
// tcb's to walk, from the state in the record.  No payload byte is read.
//   tcp_rx_acks acks(conns.count());
//   acks.run(rx_out, n, d_ack, queues, now_ns, out, d_ws, stream);   // rx_out: what tcp_rx::run wrote
class tcp_rx_acks {
    uint32_t _nconns;

public:
    // the retransmit queues (_snd.data) as a CSR (device arrays): connection c's entries are [first[c], first[c + 1])
    struct queues {
        const uint32_t* first = nullptr;  // nconns + 1
        const uint32_t* len = nullptr;    // nq: the entry's current p.len()
        const uint32_t* meta = nullptr;   // nq: data_len | (nr_transmits != 0) << 16
        const int64_t* tx = nullptr;      // nq: tx_time in ns of now_ns's clock
        uint64_t nq = 0;
    };

    // what run() writes (device arrays; <sccsum.h>, "TCP ACK fast path")
    struct outputs {
        sccsum_tcp_ack_run* run = nullptr;   // min(n, nconns), 16-byte aligned
        uint64_t* total = nullptr;           // 4: R, taken ACKs, popped entries, acked bytes
    };

    // nconns: the entries of d_ack, the table's count()
    explicit tcp_rx_acks(uint32_t nconns) : _nconns(nconns) {}

    uint32_t nconns() const noexcept { return _nconns; }

    uint64_t workspace(uint64_t n, uint64_t nq) const noexcept { return sccsum_tcp_rx_acks_workspace(n, _nconns, nq); }

    // rx, n: tcp_rx::run's outputs as they stand on the device and its n; d_ack: one sccsum_tcp_ack per
    // connection, 16-byte aligned; now_ns: the one clock_type::now() of the batch
    void run(const tcp_rx::outputs& rx, uint64_t n, const sccsum_tcp_ack* d_ack, const queues& q, int64_t now_ns,
             const outputs& out, void* d_workspace, void* stream) const {
        detail::check(sccsum_tcp_rx_acks(rx.seg, rx.first, rx.run_conn, rx.run_first, rx.total, n, d_ack, _nconns,
                                         q.first, q.len, q.meta, q.tx, q.nq, now_ns, out.run, out.total, d_workspace,
                                         stream),
                      "sccsum_tcp_rx_acks");
    }
};

// TCP rx, the passive open (<sccsum.h> sccsum_tcp_listen): what tcp::received
// does with the segments of tcp_rx's LISTEN bucket (tcp.hh:888-929) — full(),
// the RST / ACK / SYN triage, and per new connection input_handle_listen_state
// with the options parsed, the ISN, one record and the staged SYN-ACK — up to
// the first segment that needs a tcb of this very batch; from there the host
// walks in order.  Only the option bytes of the frames are read.
//   tcp_listen listen({key..., isn_m, 1500, 0});
//   listen.run(ip, rx_out, m_max, d_space, out, d_ws, stream);   // rx_out: what tcp_rx::run wrote
//   tx.run(out.synack, 32 * total[1], out.sa_off, out.sa_len, out.sa_out, total[1], tx_out, stream);
class tcp_listen {
    sccsum_tcp_listen_opts _opts;

public:
    // what run() writes (device arrays with room for m_max entries; <sccsum.h>, "TCP passive open")
    struct outputs {
        uint8_t* cls = nullptr;              // m_max
        sccsum_tcp_new* rec = nullptr;       // m_max, 16-byte aligned
        void* synack = nullptr;              // 32 m_max bytes
        uint64_t* sa_off = nullptr;          // m_max
        uint32_t* sa_len = nullptr;          // m_max
        sccsum_tcp_out* sa_out = nullptr;    // m_max
        void* rst = nullptr;                 // 20 m_max bytes
        uint32_t* rst_dst = nullptr;         // m_max
        uint64_t* total = nullptr;           // 4: taken, created, resets, dropped
    };

    explicit tcp_listen(const sccsum_tcp_listen_opts& opts) : _opts(opts) {}

    const sccsum_tcp_listen_opts& opts() const noexcept { return _opts; }
    // the batch's one clock_type::now(): microseconds since the epoch / 4
    void set_isn_m(uint32_t isn_m) noexcept { _opts.isn_m = isn_m; }

    static uint64_t workspace(uint64_t m_max) noexcept { return sccsum_tcp_listen_workspace(m_max); }

    // ip: the batch tcp_rx::run was given; rx: its outputs as they stand on the device; m_max: an upper bound of
    // the LISTEN bucket's size (tcp_rx's n always is one); d_space: 65536 words, the room left per listening port
    void run(const device_packet_batch& ip, const tcp_rx::outputs& rx, uint64_t m_max, const uint32_t* d_space,
             const outputs& out, void* d_workspace, void* stream) const {
        detail::check(sccsum_tcp_listen(_opts, ip.bytes, ip.bytes_len, ip.off, ip.n, rx.first, rx.order, rx.seg, rx.src,
                                        m_max, d_space, out.cls, out.rec, out.synack, out.sa_off, out.sa_len,
                                        out.sa_out, out.rst, out.rst_dst, out.total, d_workspace, stream),
                      "sccsum_tcp_listen");
    }
};

}  // namespace net

}  // namespace seastar
