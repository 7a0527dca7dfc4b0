/*
 * sccsum.h — C-ABI boundary of the MI355X (gfx950) batch Internet-checksum
 * engine.  Plain pointers and sizes only; every entry point returns 0 on
 * success, a positive hipError_t value for a HIP runtime failure, or a
 * negative SCCSUM_E* code; nothing throws.
 *
 * What each entry replaces in scylladb/seastar (paths relative to the
 * reference tree):
 *
 *   sccsum_spans        N x { checksummer c; [pseudo-header seed];
 *                             c.sum(data, len); c.get(); }
 *                       = ip_checksum(const void*, size_t)  src/net/ip_checksum.cc:70-74
 *                         checksummer::sum(const char*, size_t)  src/net/ip_checksum.cc:31-53
 *                         checksummer::get() const  src/net/ip_checksum.cc:55-62
 *                       as used by UDP generate  src/net/udp.cc:184-195,
 *                       TCP generate  include/seastar/net/tcp.hh:1656-1694, 1004-1016,
 *                       ICMP echo  src/net/ip.cc:471-474, demos/echo_demo.cc:76-78
 *   sccsum_ipv4_frames  N x { IPv4 header verify/generate over sizeof(ip_hdr)=20 B
 *                             src/net/ip.cc:121-127, 271-277;
 *                             length checks / trim / strip 4*ihl  src/net/ip.cc:128-140, 220-225;
 *                             L4 pseudo-header + segment  include/seastar/net/tcp.hh:876-883 }
 *   sccsum_fragments    N x checksummer::sum(const packet&)  src/net/ip_checksum.cc:64-68
 *                       (fragment lists with the odd-byte carry) + get()
 *   sccsum_ipv4_fill    the tx writers, in place on contiguous frames:
 *                       csum.sum(p); write_nbo_checksum  include/seastar/net/tcp.hh:1691-1694,
 *                       src/net/udp.cc:184-195, ipv4::send  src/net/ip.cc:266-278,
 *                       icmp::received  src/net/ip.cc:464-474
 *   sccsum_ipv4_fill_desc  the same on packets given as fragment lists, written
 *                       where the fragments lie (a tx packet: header fragment
 *                       + payload fragments); sccsum_burst_set_fill makes it
 *                       the burst queue's batch step (qp::poll_tx)
 *   sccsum_*_multi      the above for up to 16 batches (rx queues) in one launch
 *   sccsum_steer_run    N x device::hash2cpu / device::forward_dst
 *                       include/seastar/net/net.hh:287-305 (dpdk hash2qid src/net/dpdk.cc:505-508)
 *                       as interface::dispatch_packet src/net/net.cc:330-344 and
 *                       ipv4::handle_received_packet src/net/ip.cc:197 call them, after the
 *                       drops of src/net/ip.cc:121-144, plus the per-shard packet lists
 *                       their forward() calls fill; sccsum_steer_build_reta =
 *                       qp::build_sw_reta src/net/net.cc:214-231
 *   sccsum_ipv4_send    N x ipv4::send  src/net/ip.cc:244-299: the IPv4 header it prepends
 *                       (249-281) and, past the MTU (needs_frag, ip.cc:100-111), the cut
 *                       into fragments (283-294), as header + payload fragment lists —
 *                       no payload byte moves; sccsum_ipv4_send_plan = the count for one
 *   sccsum_ipv4_reasm   the reassembly branch of ipv4::handle_received_packet  src/net/ip.cc:164-220
 *                       with ipv4::frag::merge / is_complete (412-437) and packet_merger::merge
 *                       include/seastar/net/packet-util.hh:45-151, for the keys whose outcome does
 *                       not depend on arrival order, as fragment lists — no payload byte moves;
 *                       sccsum_ipv4_frag_records = the fragments of a frames batch as records
 *   sccsum_udp_rx       the end of ipv4::handle_received_packet  src/net/ip.cc:159-162, 222-227 and
 *                       ipv4_udp::received  src/net/udp.cc:45-53, 164-173: the datagrams of an IPv4
 *                       bucket grouped by channel, both headers trimmed; sccsum_udp_rx_reasm =
 *                       the same for reassembled datagrams
 *   sccsum_udp_send     N x ipv4_udp::send  src/net/udp.cc:175-197: the header in the payload's
 *                       headroom, the checksum pass's spans and seeds
 *   sccsum_pseudo_seed  ipv4_traits::{tcp,udp}_pseudo_header_checksum
 *                       include/seastar/net/ip.hh:70-75 (host arithmetic, O(1))
 *
 * Result convention (same as the reference): each 16-bit checksum is returned
 * with its bytes already in network order, i.e. storing the uint16_t to the
 * packet's checksum field writes the wire bytes (ip_checksum.cc:61,
 * tcp.hh:283-285).  A verify passes when the recomputed value is 0.
 *
 * Memory contract:
 *   - d_bytes, d_off, d_len, d_seed, d_out*, d_status are DEVICE pointers
 *     (hipMalloc / torch CUDA tensors) on the calling thread's current device.
 *   - bytes_len is the number of valid bytes at d_bytes.  The kernels read in
 *     aligned 16-byte units, so the allocation must be readable up to
 *     roundup(bytes_len, 16) (hipMalloc allocations always are).
 *   - A packet whose [off, off+len) is not inside [0, bytes_len) is not read:
 *     its outputs are 0 and its status has SCCSUM_ST_RANGE.
 *   - d_bytes must be 16-byte aligned, d_off 8-byte aligned, d_len/d_seed/d_out2 4-byte aligned,
 *     d_out 2-byte aligned.
 *   - `stream` must belong to the calling thread's current device (the one
 *     the data lives on; NULL = that device's null stream).  HIP runs a kernel
 *     on its stream's device, so each launch takes the device from the stream
 *     (hipStreamGetDevice) and sizes its grid and takes its tile-counter slot
 *     on that device; a stream of another device returns SCCSUM_EINVAL and
 *     launches nothing.  A shard thread bound to device d (sccsum_init(d))
 *     launches on streams it created while d was current.
 *   - Errors: an entry returns its own launch's error (hipLaunchKernel's);
 *     a pending HIP error from an earlier, unrelated call on the thread is
 *     left pending, neither cleared nor reported as this call's.
 *   - Launches are asynchronous on `stream` (a hipStream_t; NULL = the
 *     device's null stream), one kernel each (two for in-place fill and
 *     fragment lists).  No allocation, no memset and no host synchronisation
 *     on the launch path — sccsum_init allocates the device's pool of tile
 *     counters once; the one exception is sccsum_ipv4_fill with a NULL
 *     d_out2, whose scratch is a stream-ordered hipMallocAsync / hipFreeAsync
 *     pair on `stream` — so the calls are safe inside hipStreamBeginCapture
 *     (global or relaxed mode) and never stall another stream.  Any number
 *     of launches may be in flight, on any streams: a launch takes a counter
 *     slot no unfinished launch holds, and the kernel itself reports when it
 *     is done with it (streams may be created and destroyed freely; a
 *     destroyed stream's address reused by a new stream shares nothing).
 *     Captured launches, and launches that find no free slot, use a static
 *     tile order instead (same results, without the dynamic balance).
 *
 * Threading: Seastar's model — one reactor thread per shard, all of them
 * on one device or each on its own — is supported: any number of host
 * threads may call concurrently, each on its own streams (the counter pool
 * is shared under a per-device lock held for a few ring probes per launch).
 * Diagnostic knobs (sccsum_diag.h) are per thread.  A burst queue or a
 * pipeline object belongs to one thread; a resident engine takes steps from
 * any number of threads (its "Producers" paragraph below).
 */
#ifndef SCCSUM_H
#define SCCSUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): frames leave IP fragments' L4 alone (SCCSUM_ST_IPFRAG), L4
 * values of protocols other than TCP / UDP carry no pseudo-header, fill gained
 * SCCSUM_FILL_ICMP_ECHO ("Migration from ABI 1").
 * 3 (round 5): a launch on a stream of another device is SCCSUM_EINVAL and a
 * pending HIP error is left pending (round 4, unversioned then); the engine
 * gained SCCSUM_EIDLE, fill steps (SCCSUM_ENGINE_FILL,
 * sccsum_engine_submit_fill), one running engine per device
 * (sccsum_engine_start: SCCSUM_EBUSY), and sccsum_engine_create no longer
 * changes the caller's current device.
 * 4 (round 6): engine runs are unbounded (max_steps sizes a descriptor ring),
 * any number of threads may submit into one engine, sccsum_engine_create_opts
 * (idle and dependency limits), SCCSUM_EFAULT; the desc calls accept a NULL
 * descriptor array when no packet has fragments; sccsum_engine_stop / _destroy
 * report SCCSUM_EIDLE only when a published step was left undone.
 * 4, additive (round 7): sccsum_ipv4_fill_desc, sccsum_burst_set_fill.
 * 4, additive (round 8): sccsum_steer_* (rx steering).
 * 4, additive (round 9): sccsum_ipv4_send* (tx send).
 * 4, additive (round 10): sccsum_ipv4_frag_records, sccsum_ipv4_reasm* (rx reassembly). */
#define SCCSUM_ABI_VERSION 4

#define SCCSUM_OK 0
#define SCCSUM_EINVAL (-1)   /* bad argument (null pointer, misalignment) */
#define SCCSUM_ENODEV (-2)   /* no HIP device / device index out of range */
#define SCCSUM_EBUSY  (-3)   /* burst queue: every batch slot is in flight; poll and retry.  engine: the
                                run's steps are used up, a wait timed out, or another engine runs on the device */
#define SCCSUM_EIDLE  (-4)   /* engine: its grid gave up waiting for steps (idle limit); start a new run */
#define SCCSUM_EFAULT (-5)   /* engine: its grid stopped on an internal fault (a wait on a dependency past its
                                limit, a step it could not find); the run is over.  Never expected */

/* per-packet status bits (d_status) */
#define SCCSUM_ST_OK        0x01u /* spans: result == 0; frames: IPv4 header verifies */
#define SCCSUM_ST_L4_OK     0x02u /* frames: L4 (pseudo-header + segment) verifies */
#define SCCSUM_ST_MALFORMED 0x04u /* frames: len < 20, len < ip total length, 4*ihl > ip length, or
                                     fragment offset + ip length > 65535 (ip.cc:115-144: dropped) */
#define SCCSUM_ST_RANGE     0x08u /* [off, off+len) outside the byte buffer: not read */
#define SCCSUM_ST_IPFRAG    0x10u /* frames: an IP fragment (MF set or fragment offset != 0, ip.hh:400-402):
                                     its L4 value is not computed (0, never SCCSUM_ST_L4_OK) — the
                                     reference sums L4 over the reassembled datagram only (ip.cc:164-220) */

/* ABI version of the loaded library (== SCCSUM_ABI_VERSION it was built with). */
int sccsum_abi_version(void);

/* Static text for an error code returned by any entry point. */
const char* sccsum_strerror(int err);

/* Number of visible HIP devices. */
int sccsum_device_count(int* count);

/* The NUMA node a device's PCI function sits on (sysfs numa_node of its
 * hipDeviceGetPCIBusId address), -1 when the platform reports none.  Seastar
 * pins each shard's thread to a core and binds its memory to that core's
 * node (src/core/reactor.cc:4163, src/core/memory.cc:1898-1951); a shard
 * should drive a GPU on its own node, so its batches and pinned pools do not
 * cross the socket link ("Which GPU a shard drives"). */
int sccsum_device_numa_node(int device, int* node);

/* Bind the calling host thread to `device` (hipSetDevice), cache its
 * compute-unit count for launch sizing and, on the device's first call,
 * allocate its pool of tile counters (2048 slots, 34 MB of HBM, plus 8 KiB
 * of pinned memory the kernels report completion to; zeroed, synchronously).
 * Call it on every thread that launches; launches on a device nobody
 * initialised use the static tile order (same results). */
int sccsum_init(int device);

/* Pseudo-header partial sum exactly as ipv4_traits::*_pseudo_header_checksum
 * leaves it in a fresh checksummer (ip.hh:70-75), folded to 16 bits with
 * end-around carry.  src_host/dst_host are host-order addresses
 * (ipv4_address.ip); len is uint16_t so 65536 wraps to 0 like the reference. */
uint32_t sccsum_pseudo_seed(uint32_t src_host, uint32_t dst_host, uint8_t proto, uint16_t len);

/* Checksum n independent byte spans.
 *   d_out[i]    = checksum of d_bytes[d_off[i] .. d_off[i]+d_len[i]) started
 *                 from seed d_seed[i] (d_seed may be NULL: no seed).
 *   d_status[i] = SCCSUM_ST_OK if d_out[i] == 0 (verify); may be NULL.
 *   max_len     = upper bound of d_len[] used to pick the kernel variant
 *                 (0 = unknown; any value is correct, it only tunes speed).
 * Every uint64_t d_off[i] and every uint32_t d_len[i] is either summed
 * exactly or refused with SCCSUM_ST_RANGE: the range test is d_off > bytes_len
 * || d_len > bytes_len - d_off in 64 bits (an offset whose low 32 bits, or
 * whose wrapped end, would be in range is refused), and a span of 2^31 bytes
 * or more, up to 2^32 - 1, sums like any other (one wave scans it).  The same
 * holds for every entry point that takes d_off / d_len, in buffers wider than
 * 4 GiB too (tests/test_gpu_wide.py). */
int sccsum_spans(const void* d_bytes, uint64_t bytes_len,
                 const uint64_t* d_off, const uint32_t* d_len, const uint32_t* d_seed,
                 uint16_t* d_out, uint8_t* d_status, uint64_t n, uint32_t max_len,
                 void* stream);

/* Checksum n IPv4 frames (IPv4 header first, no Ethernet header), as the rx
 * path ipv4::handle_received_packet (ip.cc:114-229) takes them.
 *   d_out2[2i]   = IPv4 header checksum over 20 bytes (ip.cc:121-127; checked
 *                  on every frame, fragments included)
 *   d_out2[2i+1] = L4 checksum over [4*ihl, min(ip_len, len)): for TCP (6) and
 *                  UDP (17) seeded with the pseudo-header (src, dst, proto from
 *                  the header; length = that L4 span's length as uint16_t:
 *                  tcp.hh:876-883, udp.cc:184-195); for ICMP and every other
 *                  protocol the plain sum, no pseudo-header (ip.cc:471-474);
 *                  0 for an IP fragment (SCCSUM_ST_IPFRAG): the reference
 *                  checks L4 only on the reassembled datagram — sum that with
 *                  sccsum_spans_desc over the fragments' payloads and the
 *                  pseudo-header seed ("Fragments")
 *   For generate, pass frames whose checksum fields are zero and store the
 *   outputs; for verify, pass received frames and test the status bits.
 *   d_status may be NULL.  max_len as for sccsum_spans.
 *   Verify only: d_out2 may be NULL when d_status is given — the launch then
 *   writes 1 status byte per frame instead of 4 + 1 (the reference's verify
 *   keeps only get() != 0: ip.cc:121-127, tcp.hh:876-883).  The same holds
 *   per batch in sccsum_ipv4_frames_multi.  Neither given: SCCSUM_EINVAL. */
int sccsum_ipv4_frames(const void* d_bytes, uint64_t bytes_len,
                       const uint64_t* d_off, const uint32_t* d_len,
                       uint16_t* d_out2, uint8_t* d_status, uint64_t n, uint32_t max_len,
                       void* stream);

/* ---- Several batches in one launch ------------------------------------------
 * Up to SCCSUM_MAX_BATCHES independent batches (e.g. the rx queues of a shard,
 * or a step's tx and rx halves) checksummed by ONE kernel launch: each batch
 * is exactly what sccsum_spans / sccsum_ipv4_frames would compute for it (its
 * own bytes, offsets, lengths, seeds and outputs; same memory contract), but
 * the launch's ramp and drain (~6-7 us on MI355X) are paid once.  batches is
 * a HOST array (read before the call returns); empty batches are skipped.
 * Frames take no seeds (d_seed must be NULL).  SCCSUM_EINVAL for nbatch >
 * SCCSUM_MAX_BATCHES or a bad batch. */
#define SCCSUM_MAX_BATCHES 16

typedef struct sccsum_batch {
    const void* d_bytes;
    uint64_t bytes_len;
    const uint64_t* d_off;
    const uint32_t* d_len;
    const uint32_t* d_seed; /* spans: optional per-packet seed; frames: NULL */
    void* d_out;            /* spans: uint16_t[n]; frames: uint16_t[2n] */
    uint8_t* d_status;      /* optional */
    uint64_t n;
} sccsum_batch;

int sccsum_spans_multi(const sccsum_batch* batches, uint32_t nbatch, uint32_t max_len, void* stream);
int sccsum_ipv4_frames_multi(const sccsum_batch* batches, uint32_t nbatch, uint32_t max_len, void* stream);

/* ---- Resident engine: steps streamed into a running grid -------------------
 * A launch pays a fixed cost — the grid's ramp, the drain of its last tiles
 * and the kernel boundary, ~18-21 us on MI355X — on every call.
 * An engine launches ONE grid that stays resident and takes STEPS from the
 * host while it runs, the way Seastar's reactor keeps polling its queues
 * (src/core/reactor.cc:3543-3550): each step is up to SCCSUM_ENGINE_MAX_BATCHES
 * batches (a step's tx and rx halves, a shard's rx queues), computed exactly
 * as sccsum_*_multi would compute them, and its tiles flow into the same
 * grid without a boundary.  Per step the engine reports completion; its
 * results are written through to device memory, so a DEVICE-TO-HOST copy
 * (hipMemcpy / hipMemcpyAsync to host memory, which a copy engine runs) may
 * read them as soon as sccsum_engine_wait returns for the step.  Anything
 * that runs as a kernel on the device — another library launch, a torch op,
 * a device-to-device copy that HIP runs as a blit kernel — waits for the run
 * to stop (see "Sharing the device" below).
 *
 *   sccsum_engine_create(device, mode, max_steps, max_in_flight, &e)
 *       mode SCCSUM_PIPE_IPV4 (frames) or SCCSUM_PIPE_SPANS, frames may add
 *       SCCSUM_ENGINE_FILL (the run also takes fill steps; max_in_flight >= 2);
 *       max_steps (1..65536, rounded up to a power of two, at least 2) = the
 *       slots of the engine's descriptor RING (512 B of pinned memory and as
 *       much device memory each): a run takes any number of steps, a slot
 *       being reused once its step is done; at most min(max_in_flight (1..256),
 *       max_steps) steps submitted and not yet done.  Allocates on `device`;
 *       the calling thread's current device is left as it was.
 *   sccsum_engine_create_opts(device, mode, &opts, &e)   the same with every
 *       limit given (sccsum_engine_opts; a 0 field takes its default)
 *   sccsum_engine_start(e, stream)      launch the grid on `stream` (a run);
 *       `stream` belongs to the engine's device, which must be the calling
 *       thread's current device (sccsum_init(device)).  SCCSUM_EBUSY when
 *       another engine of this process runs on the device.
 *   sccsum_engine_submit(e, batches, nbatch, max_len, timeout_ns, &step)
 *       publish one step; waits (spinning, up to timeout_ns) while the
 *       in-flight limit's steps are pending.  SCCSUM_EBUSY: the wait timed
 *       out; SCCSUM_EINVAL: the engine is not running (never started, or
 *       stopped); SCCSUM_EIDLE / SCCSUM_EFAULT: the run is over.
 *       max_len (0 = unknown) caps the mean packet length the step's tiles
 *       are sized by (bytes_len / n otherwise, too big for a batch that is a
 *       slice of a larger buffer).  The engine always runs the flat kernel, so
 *       sparse layouts give exact results but belong on the launches, whose
 *       row kernel reads them faster.  Frames take no seeds.  A step whose
 *       batches are all empty is done once the grid has taken it in.
 *   sccsum_engine_submit_fill(e, batches, nbatch, max_len, mode, timeout_ns, &step)
 *       an in-place fill (sccsum_ipv4_fill's SCCSUM_FILL_L4 and/or
 *       SCCSUM_FILL_ICMP_ECHO, optionally | SCCSUM_FILL_IP) of every batch
 *       (d_bytes is written; each batch's d_out, required here, gets the
 *       values stored and d_status the status bits).  A fill of at most
 *       524 288 frames (sccsum_set_fill_single_max) is ONE step whose tiles
 *       store the fields themselves; a larger one is two consecutive steps: a
 *       generate step into d_out and a store step whose tiles wait for it and
 *       write the values into the frames' fields (both or neither are
 *       published).  *step = the fill's last step: once it is done the frames
 *       are wire-ready in device memory and d_out holds the values stored.  No
 *       other step may write a fill's d_out (nor its frames) before the fill is
 *       done.  max_len as for submit.
 *   sccsum_engine_wait(e, step, timeout_ns)   0 once the step is done;
 *       SCCSUM_EBUSY on time out, SCCSUM_EIDLE / SCCSUM_EFAULT if the grid
 *       gave up before the step was done
 *   sccsum_engine_stop(e)               no more steps: the grid leaves once the
 *       published steps are done (synchronise `stream` to wait for it).
 *       SCCSUM_EIDLE (SCCSUM_EFAULT) when the grid had already given up with a
 *       published step not done: after the stream sync,
 *       sccsum_engine_wait(e, step, 0) still answers for every step of the
 *       run's last max_steps (0 done, the give-up's code otherwise)
 *   sccsum_engine_destroy(e)            stops and synchronises a running engine;
 *       SCCSUM_EIDLE (SCCSUM_EFAULT) if its last run left a published step
 *       undone (a give-up after every step was done loses nothing: 0)
 *
 * Producers.  Any number of host threads may submit into one running engine
 * and wait on its steps — the shards that share a GPU, each with its own
 * batches: a step's number, first tile and descriptor are taken and published
 * under the engine's lock (a few hundred ns, no device call), so steps are
 * published in the order their submits took the lock, and a submit that waits
 * for room waits outside it.  The in-flight limit is the engine's, shared by
 * every producer; opts.producer_in_flight adds one per producer thread, so
 * that no shard holds the whole shared limit: a thread's submit past it first
 * waits (within its timeout) for that thread's oldest step not yet done.  (A
 * fill counts once: by its last step.)  Start, stop and destroy belong to the engine's owner (a
 * submit after stop returns SCCSUM_EINVAL; destroy only after every producer's
 * last call has returned).
 *
 * Sharing the device.  The grid holds the device's compute units while it
 * runs (every CU, all of their LDS): kernels that other threads or streams
 * launch on the device — this library's launches included — queue until the
 * run stops, and then complete.  So one engine runs per device at a time
 * (per process: a second start returns SCCSUM_EBUSY until the first run's
 * stop), and the shards of a GPU submit into its one engine (Producers) or
 * use launches while no engine runs there.  A grid given no new step (and no
 * stop) for its idle limit (default 1 s) leaves on its own, and every later
 * call on that run returns SCCSUM_EIDLE: the limit counts from the last step
 * the grid received, so steady light traffic never trips it. */
#define SCCSUM_ENGINE_MAX_BATCHES 4
#define SCCSUM_ENGINE_FILL 0x100 /* sccsum_engine_create mode flag: the run takes fill steps too */
typedef struct sccsum_engine sccsum_engine;
typedef struct sccsum_engine_opts {
    uint32_t ring_slots;    /* descriptor ring slots, 1..65536 (a power of two, at least 2, above); 0 = 1024 */
    uint32_t max_in_flight; /* steps submitted and not yet done, 1..256 (fill engines: >= 2); 0 = 8 */
    uint32_t idle_ms;       /* the grid leaves after this long without a new step (SCCSUM_EIDLE),
                               1..3 600 000; 0 = 1000 */
    uint32_t dep_ms;        /* limit of a step's wait on the step it depends on (a fill's store step on its
                               generate step, a barrier; SCCSUM_EFAULT past it), 1..3 600 000; 0 = 2000 */
    uint32_t producer_in_flight; /* one producer thread's own steps submitted and not yet done,
                                    1..max_in_flight; 0 = no limit of its own (Producers) */
} sccsum_engine_opts;
int sccsum_engine_create(int device, int mode, uint32_t max_steps, uint32_t max_in_flight, sccsum_engine** out);
int sccsum_engine_create_opts(int device, int mode, const sccsum_engine_opts* opts, sccsum_engine** out);
int sccsum_engine_start(sccsum_engine* e, void* stream);
int sccsum_engine_submit(sccsum_engine* e, const sccsum_batch* batches, uint32_t nbatch, uint32_t max_len,
                         uint64_t timeout_ns, uint64_t* step);
int sccsum_engine_submit_fill(sccsum_engine* e, const sccsum_batch* batches, uint32_t nbatch, uint32_t max_len,
                              uint32_t mode, uint64_t timeout_ns, uint64_t* step);
int sccsum_engine_wait(sccsum_engine* e, uint64_t step, uint64_t timeout_ns);
int sccsum_engine_stop(sccsum_engine* e);
int sccsum_engine_destroy(sccsum_engine* e);

/* Checksum n packets that are FRAGMENT LISTS, like checksummer::sum(const
 * packet&) (src/net/ip_checksum.cc:64-68): packet i is the concatenation of
 * fragments d_pkt_first[i] .. d_pkt_first[i+1]-1, fragment j being
 * d_bytes[d_frag_off[j] .. +d_frag_len[j]) (any order, any alignment; DPDK
 * multi-segment mbufs, virtio mergeable buffers).  A fragment that starts at
 * an odd offset of its packet contributes byte-swapped, exactly the
 * reference's `odd` carry.  d_pkt_first has n+1 nondecreasing entries ending
 * at nfrag; d_seed / d_status optional as for sccsum_spans.  d_workspace:
 * device scratch of sccsum_fragments_workspace(nfrag) bytes, 16-byte aligned.
 * A packet with a fragment outside the buffer (or a bad d_pkt_first range)
 * gets 0 and SCCSUM_ST_RANGE. */
int sccsum_fragments(const void* d_bytes, uint64_t bytes_len,
                     const uint64_t* d_frag_off, const uint32_t* d_frag_len, uint64_t nfrag,
                     const uint32_t* d_pkt_first, const uint32_t* d_seed,
                     uint16_t* d_out, uint8_t* d_status, uint64_t n, uint32_t max_frag_len,
                     void* d_workspace, void* stream);
uint64_t sccsum_fragments_workspace(uint64_t nfrag);

/* sccsum_ipv4_fill modes */
/* ---- RSS: the Toeplitz hash the rx path steers flows by --------------------
 * include/seastar/net/toeplitz.hh:78-98 over the forward_hash the stack
 * builds for a frame (net.hh:53-75):
 *   SCCSUM_RSS_DISPATCH (net.cc:330-341 -> ip.cc:77-92): src + dst IP, then
 *     for an atomic TCP / UDP datagram (MF clear, fragment offset 0) the 4
 *     port bytes at frame offset 20 (sizeof(ip_hdr): options not skipped),
 *     if the frame holds the TCP (20 B) / UDP (8 B) header there
 *     (tcp.hh:852-862, udp.cc:153-161);
 *   SCCSUM_RSS_REASSEMBLED (ip.cc:186-197): src + dst IP, then the ports at
 *     4*ihl when the L4 part (up to min(ip total length, len)) holds the
 *     TCP / UDP header.
 * key: HOST pointer, key_len >= 4 bytes (the reference's defaults are 40 and
 * 52 bytes, toeplitz.hh:52-71; only the first 16 can reach a 12-byte input).
 * d_hash[i] = the 32-bit hash; 0 for a malformed frame (shorter than 20 B, or
 * REASSEMBLED with 4*ihl past the datagram: status SCCSUM_ST_MALFORMED) or an
 * out-of-range one (SCCSUM_ST_RANGE). */
#define SCCSUM_RSS_DISPATCH    0
#define SCCSUM_RSS_REASSEMBLED 1

/* RSS hashes alone (one thread per frame, reads ~28 header bytes each). */
int sccsum_ipv4_rss(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                    const uint8_t* key, uint32_t key_len, int mode, uint32_t* d_hash, uint8_t* d_status, uint64_t n,
                    void* stream);

/* sccsum_ipv4_frames plus the RSS hash of every frame in the same pass (the
 * flat kernel computes it from the header bytes it already holds; no extra
 * HBM traffic beyond the 4-byte hash). */
int sccsum_ipv4_frames_rss(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                           uint16_t* d_out2, uint8_t* d_status, uint64_t n, uint32_t max_len, const uint8_t* key,
                           uint32_t key_len, int rss_mode, uint32_t* d_hash, void* stream);

/* ---- Rx steering: hash2cpu for a batch + its stable partition by shard ------
 * What the rx path does with a packet's hash, for a whole batch on the device:
 * device::forward_dst (net.hh:291-300) / device::hash2cpu (net.hh:301-305)
 * give every packet its destination shard, and the batch's packet indices are
 * grouped by shard in arrival order — the per-shard lists that
 * interface::dispatch_packet's forward() (net.cc:330-344) and
 * ipv4::handle_received_packet (ip.cc:197) build one packet at a time.  It
 * consumes only the d_hash / d_status arrays the RSS and frames launches
 * write, so it follows any launch form.
 *
 * sccsum_steer_map (all tables are HOST memory, read by sccsum_steer_create /
 * sccsum_steer_dest only):
 *   hash2qid(hash) = redir[hash & (redir_size - 1)] when redir_size != 0
 *                    (dpdk.cc:505-508), else hash % hw_queues (net.hh:287-289)
 *   forward_dst(q, hash) = sw_reta[q][(hash >> table_bits) % 128] when queue q
 *                    has a _sw_reta, else q itself (a queue index past
 *                    hw_queues is a proxy queue: it never has one)
 *   SCCSUM_STEER_DISPATCH: dest = forward_dst(src_cpu, hash)
 *   SCCSUM_STEER_HASH2CPU: dest = forward_dst(hash2qid(hash), hash)
 * A hash of 0 (what the reference and the RSS kernels give a packet they
 * cannot hash) steers like any other.
 *
 * sccsum_steer_create validates every table entry (redir < hw_queues, sw_reta
 * < ncpu, a queue without a _sw_reta < ncpu since it maps to itself) and
 * copies the tables to `device`; control plane: it allocates and
 * synchronises, and leaves the calling thread's current device as it was.
 * The object is immutable: any number of threads and streams may run it.
 *
 * sccsum_steer_run, packet i of n:
 *   dropped when d_status is given and (d_status[i] & need) != need ||
 *   (d_status[i] & reject) != 0 — the caller's policy, e.g. need =
 *   SCCSUM_ST_OK, reject = SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE for the
 *   frames the reference drops before it steers (ip.cc:121-144); with
 *   d_status NULL nothing is dropped and need / reject must be 0.
 *   d_cpu[i]   = its shard, 0xFF when dropped; may be NULL.
 *   d_first    = ncpu + 2 entries, required: d_order[d_first[c] ..
 *                d_first[c + 1]) are shard c's packets, bucket c = ncpu the
 *                dropped ones, d_first[ncpu + 1] = n.
 *   d_order[n] = packet indices grouped by bucket ascending, ascending inside
 *                a bucket (a STABLE partition: a flow's packets keep their
 *                order); may be NULL: counts only, no scatter pass.
 *   d_workspace: sccsum_steer_workspace(s, n) bytes of device scratch, 16-byte
 *                aligned; d_hash, d_order, d_first 4-byte aligned.
 *   Every output is a function of the inputs alone (no atomic decides a
 *   position): two runs give identical bytes.
 * Three small kernels on `stream` (count, scan, scatter; the scan is two past
 * 31 shards), one chain of plain dependent launches, no allocation, no memset,
 * no host synchronisation: capturable.  `stream` must belong to
 * the object's device (NULL = the current device's null stream, which must be
 * that device): SCCSUM_EINVAL otherwise.  n == 0 writes d_first (zeros) when
 * it is given and is SCCSUM_OK without device work when it is NULL; n > 2^32-1
 * is SCCSUM_EINVAL (indices are 32-bit), like every argument error before any
 * device work.  DISPATCH from a src_cpu that has no _sw_reta sends every
 * packet to src_cpu, which must then be < ncpu. */
typedef struct sccsum_steer sccsum_steer;
typedef struct sccsum_steer_map {
    uint32_t ncpu;          /* destination shards 0..ncpu-1; 1..255 (0xFF marks a dropped packet) */
    uint32_t hw_queues;     /* 1..256: device::hw_queues_count() */
    uint32_t table_bits;    /* device::_rss_table_bits, 0..31 */
    uint32_t redir_size;    /* 0, or a power of two 1..512: the dpdk _redir_table's size */
    const uint8_t* redir;   /* redir_size entries < hw_queues; NULL iff redir_size == 0 */
    const uint8_t* sw_reta; /* [hw_queues][128] entries < ncpu: row q = queue q's _sw_reta */
    const uint8_t* sw_reta_set; /* [hw_queues] 0/1: queue q has a _sw_reta (its row is ignored when 0);
                                   NULL = every queue has one */
} sccsum_steer_map;

#define SCCSUM_STEER_DISPATCH 0 /* forward_dst(src_cpu, hash): dispatch_packet, net.cc:330-344 */
#define SCCSUM_STEER_HASH2CPU 1 /* forward_dst(hash2qid(hash), hash): ip.cc:197, tcp.hh:839 */

int sccsum_steer_create(int device, const sccsum_steer_map* map, sccsum_steer** out);
int sccsum_steer_destroy(sccsum_steer* s);
uint64_t sccsum_steer_workspace(const sccsum_steer* s, uint64_t n);
int sccsum_steer_run(const sccsum_steer* s, int mode, uint32_t src_cpu, const uint32_t* d_hash,
                     const uint8_t* d_status, uint32_t need, uint32_t reject, uint64_t n, uint8_t* d_cpu,
                     uint32_t* d_order, uint32_t* d_first, void* d_workspace, void* stream);

/* One hash through a map on the host (O(1), no table validation: the entries
 * it reads are returned as they are); 0xFFFFFFFF for a NULL map, a bad scalar
 * field or a bad mode. */
uint32_t sccsum_steer_dest(const sccsum_steer_map* map, int mode, uint32_t src_cpu, uint32_t hash);

/* qp::build_sw_reta (net.cc:214-231) with the same float arithmetic: the
 * 128-entry table of n cpus (strictly ascending, as the reference's std::map
 * iterates; each <= 254) with weights >= 0.  SCCSUM_EINVAL when the weights
 * do not fill all 128 entries (their sum is 0), which the reference would
 * leave unset. */
int sccsum_steer_build_reta(const uint32_t* cpus, const float* weights, uint32_t n, uint8_t reta[128]);

#define SCCSUM_FILL_IP       0x01u /* IPv4 header checksum, field at +10 (ip.cc:266-278) */
#define SCCSUM_FILL_L4        0x02u /* full TCP/UDP checksum: pseudo-header + segment (udp.cc:190-192,
                                       tcp.hh:1691-1692 without tx offload) */
#define SCCSUM_FILL_L4_PSEUDO 0x04u /* tx-offload partial: the folded pseudo-header alone, i.e. the
                                       reference's `~csum.get()` (udp.cc:188-189, tcp.hh:1688-1689) */
#define SCCSUM_FILL_TSO       0x08u /* with L4_PSEUDO: TCP pseudo-header length 0 (tcp.hh:1674-1676) */
#define SCCSUM_FILL_ICMP_ECHO 0x10u /* ICMP echo request -> echo reply in place: type 0, code 0, checksum
                                       over the ICMP message, no pseudo-header (icmp::received,
                                       ip.cc:464-474); other ICMP types are left alone */

/* GENERATE checksums for n IPv4 frames and STORE them in the frames, in
 * place: wire-ready frames, the tx half of the native stack.  Each checksum
 * is computed as if its own field were zero, as the reference does (fresh
 * headers are value-initialised, packet.hh:586-589; ip.cc:270), so the
 * fields' current contents do not matter.  The L4 field is UDP +6 / TCP +16
 * (ICMP +2 with SCCSUM_FILL_ICMP_ECHO) after 4*ihl; other protocols' L4 is
 * left alone, as is any frame that is malformed (as in sccsum_ipv4_frames),
 * too short to hold the field, or whose ihl is below 5 (its L4 header would
 * overlap the 20-byte IP header; ipv4::send always writes ihl 5, ip.cc:249).  An IP fragment gets the IP header checksum
 * only (ipv4::send checksums each fragment's header, ip.cc:256-278, after the
 * L4 writer summed the whole datagram, ip.cc:283-294): its L4 bytes — the
 * first fragment's L4 header, a later fragment's payload — are never written.
 *   mode: SCCSUM_FILL_IP and/or one of SCCSUM_FILL_L4 / SCCSUM_FILL_L4_PSEUDO
 *         (| SCCSUM_FILL_TSO), and/or SCCSUM_FILL_ICMP_ECHO (not with
 *         L4_PSEUDO).  FILL_L4 and FILL_ICMP_ECHO read every byte (the flat
 *         kernel generates into d_out2, then a second pass stores the
 *         fields); the others read only the 20-byte header.
 *   d_out2[2i] / [2i+1] = the IP / L4 values stored (0 where nothing was
 *         stored); may be NULL: FILL_L4 / FILL_ICMP_ECHO then hand the values
 *         between the passes in a stream-ordered allocation (hipMallocAsync /
 *         hipFreeAsync on `stream`; ABI 2 as first released in round 3
 *         refused NULL here).
 *   d_status[i] = SCCSUM_ST_OK if the IP field was written, SCCSUM_ST_L4_OK
 *         if the L4 field was written, plus MALFORMED / RANGE / IPFRAG; may
 *         be NULL.
 * Frames must not overlap each other. */
int sccsum_ipv4_fill(void* d_bytes, uint64_t bytes_len,
                     const uint64_t* d_off, const uint32_t* d_len,
                     uint16_t* d_out2, uint8_t* d_status, uint64_t n, uint32_t max_len,
                     uint32_t mode, void* stream);

/* Wait for all work queued on `stream`. */
int sccsum_sync(void* stream);

/* ---------------------------------------------------------------------------
 * Host pipeline: batches that live in HOST memory (DPDK mbuf pools, socket
 * buffers).  The batch is cut into chunks of at most chunk_packets packets /
 * chunk_bytes bytes; each chunk is copied to HBM on a copy stream
 * (hipMemcpyAsync, pinned staging), checksummed on a compute stream and its
 * results copied back, with `depth` chunks in flight so the copies overlap
 * the kernels.  The device work is the same sccsum_spans / sccsum_ipv4_frames.
 * ------------------------------------------------------------------------- */
typedef struct sccsum_pipeline sccsum_pipeline;

#define SCCSUM_PIPE_SPANS 0
#define SCCSUM_PIPE_IPV4  1

#define SCCSUM_GATHER_NONE    0 /* copy each chunk's covering byte range as it lies */
#define SCCSUM_GATHER_HOST    1 /* pack packets into pinned staging on the host first */
#define SCCSUM_GATHER_STRIDED 2 /* packets at one pitch (mbuf slots): one 2D DMA of each slot's packet bytes */
#define SCCSUM_GATHER_ZERO_COPY 3 /* no copies: the kernel reads each packet in place (host_bytes pinned / registered) */

/* Allocate device buffers and pinned staging for `depth` chunks on `device`. */
int sccsum_pipeline_create(int device, uint64_t chunk_bytes, uint32_t chunk_packets, int depth,
                           sccsum_pipeline** out);

/* Checksum n packets at host_bytes[host_off[i] .. +host_len[i]) (all HOST
 * pointers; host_bytes should be pinned — sccsum_host_alloc — unless gather
 * is 1).  gather = 0: each chunk's covering byte range is copied as it lies
 * (e.g. whole mbuf slots, headers and headroom included); gather = 1: the
 * packets are first packed into pinned staging on the host (only packet bytes
 * cross PCIe); gather = 2: where a chunk's packets sit at one pitch P (the
 * slots of an mbuf pool, dpdk.cc:139-156) and none is longer than P, one 2D
 * DMA (hipMemcpy2DAsync) copies the first W bytes of each slot, W = the
 * chunk's longest packet — only packet bytes cross PCIe, with no host copy;
 * other chunks are copied as they lie; gather = 3: nothing is copied — one
 * fragment-list launch per chunk reads every packet in place over PCIe
 * (packet bytes only) and writes its results to pinned staging; host_bytes
 * must be pinned or registered (SCCSUM_EINVAL otherwise, checked with
 * hipPointerGetAttributes on both ends).  mode = SCCSUM_PIPE_SPANS (host_seed optional, host_out[n]) or
 * SCCSUM_PIPE_IPV4 (host_out[2n]); host_status optional.  Returns when all
 * results are in host_out.  host_len is the size of the host_bytes area. */
int sccsum_pipeline_run(sccsum_pipeline* p, int mode, int gather, const void* host_bytes, uint64_t host_len,
                        const uint64_t* host_off, const uint32_t* host_lens, const uint32_t* host_seed,
                        uint64_t n, uint32_t max_len, uint16_t* host_out, uint8_t* host_status);

int sccsum_pipeline_destroy(sccsum_pipeline* p);

/* ---- Burst queue: the batching hook at the qp boundary ----------------------
 * The native stack checksums packet by packet on the shard's reactor thread;
 * qp::poll_tx refills up to 128 packets per poll (src/net/net.cc:81-105) and
 * DPDK rx hands over bursts of 32 (src/net/dpdk.cc:2190-2204).  A burst queue
 * accumulates such packets from HOST memory into GPU batches and completes
 * them asynchronously.  It is shaped like a reactor::poller (net.cc:109):
 * every call is non-blocking except sccsum_burst_drain, and sccsum_burst_poll
 * reports whether it did work.  One queue per shard / thread; not thread-safe.
 *
 * mode: SCCSUM_PIPE_SPANS (each packet's sum seeded with its seed, results
 * [count]) or SCCSUM_PIPE_IPV4 (frames: IPv4 header + L4 checksums, results
 * [2*count]).  A batch launches when it holds batch_packets packets or no room
 * for the next one, or on the first poll after max_delay_ns.  depth = batch
 * slots (staging + device buffers each). */
typedef struct sccsum_burst sccsum_burst;

/* Completion, called from sccsum_burst_poll / _drain on the caller's thread:
 * the packets with tickets first_ticket .. first_ticket + count - 1, in submit
 * order; results / status point into the queue's pinned memory, valid until
 * the callback returns.  The callback may submit (a queue never reuses the
 * batch being delivered before the callback returns); poll, drain and
 * destroy called from inside it return SCCSUM_EINVAL and do nothing. */
typedef void (*sccsum_burst_done_fn)(void* user, uint64_t first_ticket, uint32_t count, const uint16_t* results,
                                     const uint8_t* status);

/* batch_bytes: 64 .. 4 GiB - 16 (a batch's byte offsets are 32-bit);
 * depth: 1 .. 64 slots.  SCCSUM_EINVAL otherwise. */
int sccsum_burst_create(int device, int mode, uint64_t batch_bytes, uint32_t batch_packets, uint64_t max_delay_ns,
                        int depth, sccsum_burst_done_fn fn, void* user, sccsum_burst** out);

/* One piece of a packet, in the layout of seastar::net::fragment {char* base;
 * size_t size;} (include/seastar/net/packet.hh:43-46): a packet's
 * fragment_array() / nr_frags() (packet.hh:245-247) pass as they are. */
typedef struct sccsum_fragment {
    const void* base;
    size_t size;
} sccsum_fragment;

/* Stage one packet given as its fragments (checksummer::sum(const packet&)
 * over the fragments in order, ip_checksum.cc:64-68): they are copied into
 * pinned staging now, so the caller may reuse them on return.  *ticket (may be
 * NULL) identifies the packet in the completion.  seed: SCCSUM_PIPE_SPANS only.
 * SCCSUM_EBUSY: every slot is in flight (poll, then retry); SCCSUM_EINVAL: a
 * packet longer than a batch. */
int sccsum_burst_submit(sccsum_burst* b, const sccsum_fragment* frags, uint32_t nfrag, uint32_t seed,
                        uint64_t* ticket);

/* Zero-copy submit: as sccsum_burst_submit, but the fragments lie in memory
 * the device can read at the same address (see sccsum_gather: pinned or
 * hipHostRegister'd host memory, or device memory) and must stay untouched
 * until the packet's completion.  Only a descriptor is recorded; the batch's
 * launch gathers the bytes on the device (over PCIe for host memory), so no
 * host thread copies packet bytes.  Both submits may be mixed in one queue.
 * SCCSUM_EINVAL also when a packet has more than 4 * batch_packets fragments. */
int sccsum_burst_submit_mapped(sccsum_burst* b, const sccsum_fragment* frags, uint32_t nfrag, uint32_t seed,
                               uint64_t* ticket);

/* Reactor poller: launch the open batch if full or aged; deliver every
 * finished batch.  *did_work (may be NULL) = 1 when it launched or delivered.
 * If a launch fails (an error code from any call that launches: submit, poll,
 * drain), its batch stays staged, nothing of it still runs on the device, and
 * the next poll / drain launches it again. */
int sccsum_burst_poll(sccsum_burst* b, int* did_work);

/* Tx form of a SCCSUM_PIPE_IPV4 queue: while fill_mode (sccsum_ipv4_fill's
 * mode bits and rules) is set, every batch is ONE sccsum_ipv4_fill_desc launch
 * on the fragments where they lie, whatever sccsum_set_burst_fused says: at
 * a packet's completion its fragments hold the generated checksums (wire-ready
 * mbufs: the hook for qp::poll_tx, net.cc:81-105), and the callback gets the
 * values stored and the fill status bits.  The fragments are WRITTEN, so only
 * sccsum_burst_submit_mapped takes packets (sccsum_burst_submit, whose bytes
 * are copies, returns SCCSUM_EINVAL), they must be writable by the device, and
 * no two fragments of a batch may overlap.  fill_mode 0 returns to values
 * only.  SCCSUM_EINVAL: a SCCSUM_PIPE_SPANS queue or a bad mode; SCCSUM_EBUSY:
 * a packet is staged or a batch in flight (drain first). */
int sccsum_burst_set_fill(sccsum_burst* b, uint32_t fill_mode);

/* Launch what is staged, wait for every batch in flight, deliver them all. */
int sccsum_burst_drain(sccsum_burst* b);

int sccsum_burst_destroy(sccsum_burst* b);

/* Gather: copy n fragments into one device buffer, d_dst[dst_off ..
 * +len) = src[0 .. len), for every descriptor (one kernel).  src may be device
 * memory or pinned host memory the device can read at the same address
 * (sccsum_host_alloc / hipHostMalloc; hipHostRegister'd memory such as a DPDK
 * mempool, registered once) — then the bytes cross PCIe without a host thread
 * touching them.  Any alignment; destinations must not overlap.  d_desc is a
 * DEVICE array (8-byte aligned).  A descriptor with src == NULL is skipped
 * (its bytes are already in place). */
typedef struct sccsum_gather_desc {
    const void* src;
    uint32_t dst_off;
    uint32_t len;
} sccsum_gather_desc;

int sccsum_gather(const sccsum_gather_desc* d_desc, uint64_t n, void* d_dst, void* stream);

/* Packets as fragment lists, summed where the fragments lie (one kernel, each
 * byte read once — over PCIe for pinned / registered host memory — with no
 * gather into a batch first): checksummer::sum(const packet&)
 * (ip_checksum.cc:64-68) for packets whose fragments may be anywhere the
 * device can read.  Packet p (p < n) has the fragments d_desc[d_first[p] ..
 * d_first[p+1]) (d_first has n + 1 entries), which must tile its bytes in
 * order: fragment j holds packet bytes [dst_off_j - d_off[p], + len_j), so
 * the first starts at dst_off = d_off[p] and the lengths add up to d_len[p].
 * A fragment with src == NULL lies at d_stage + dst_off (bytes already in a
 * device batch; d_stage may be NULL when no fragment uses it).  A packet whose
 * fragments do not tile it gets result 0 and status SCCSUM_ST_RANGE; the
 * d_first entries themselves must index inside d_desc (not checked: the
 * descriptor count is not an argument).  d_desc may be NULL when no packet has
 * a fragment (every packet empty): each packet then has zero fragments, so an
 * empty one gets the empty sum and a non-empty one 0 + SCCSUM_ST_RANGE.
 * Results and status as sccsum_spans / sccsum_ipv4_frames (frames: IPv4
 * header + L4, the header may be split across fragments).  d_desc, d_first,
 * d_off, d_len, d_seed, d_out, d_status: device arrays (aligned to their
 * element size, d_desc to 8).  max_len as for sccsum_spans: a hint, the
 * upper bound of d_len[] if known (0 = unknown); any value is correct, it only
 * picks how many 16-byte units a lane loads per pass over a fragment.
 * Any d_off and any d_len value is either summed exactly or refused with
 * SCCSUM_ST_RANGE: dst_off is compared with the 64-bit d_off (+ the bytes
 * before the fragment), so a d_off past 2^32 whose low 32 bits equal dst_off
 * does not tile; packet and fragment lengths up to 2^32 - 1 sum exactly, and
 * src is a full 64-bit address. */
int sccsum_spans_desc(const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off,
                      const uint32_t* d_len, const uint32_t* d_seed, const void* d_stage, uint16_t* d_out,
                      uint8_t* d_status, uint64_t n, uint32_t max_len, void* stream);
int sccsum_ipv4_frames_desc(const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off,
                            const uint32_t* d_len, const void* d_stage, uint16_t* d_out2, uint8_t* d_status,
                            uint64_t n, uint32_t max_len, void* stream);

/* sccsum_ipv4_fill on fragment lists: GENERATE the checksums of n IPv4 packets
 * given as for sccsum_ipv4_frames_desc and STORE them where the fragments lie
 * — the call WRITES through desc.src (through d_stage + dst_off for a fragment
 * with src == NULL), so that memory is device memory or pinned / registered
 * host memory the device can write; over PCIe the bytes are visible to the
 * host once `stream` is synchronised.  One kernel, one wave per packet: it
 * decodes the header (which may be split), sums with every field counted as
 * zero — what the fields held does not matter — and stores at most six bytes
 * itself (IP +10/+11, the L4 field, an echo reply's type and code); a field's
 * two bytes may lie in different fragments.  mode, its validity, the fields,
 * the frames that are skipped, d_out2 and d_status (each may be NULL) are
 * exactly sccsum_ipv4_fill's; FILL_IP alone and FILL_L4_PSEUDO (| FILL_TSO)
 * read only header bytes, and FILL_L4 / FILL_ICMP_ECHO read the payload only
 * of packets whose field they write.  A packet whose fragments do not tile it
 * is not written: values 0, status SCCSUM_ST_RANGE.  No two fragments of a
 * batch may overlap.  The mode is checked first (SCCSUM_EINVAL), then n == 0
 * is SCCSUM_OK; pointer / alignment errors and a stream of another device are
 * SCCSUM_EINVAL before any device work. */
int sccsum_ipv4_fill_desc(const sccsum_gather_desc* d_desc, const uint32_t* d_first, const uint64_t* d_off,
                          const uint32_t* d_len, void* d_stage, uint16_t* d_out2, uint8_t* d_status,
                          uint64_t n, uint32_t max_len, uint32_t mode, void* stream);

/* ---- Tx send: ipv4::send for a batch of L4 datagrams ---------------------------
 * What ipv4::send (ip.cc:244-299) does to one L4 datagram, for a whole batch on
 * the device: the 20-byte IPv4 header it prepends and, for a datagram that does
 * not fit the MTU (needs_frag, ip.cc:100-111), the cut into pieces.  Like the
 * reference, which shares the payload (p.share(offset, can_send)) and prepends
 * a header, NO payload byte moves: per wire frame the call writes one header and
 * two sccsum_gather_desc records, so its outputs are the arguments of
 * sccsum_ipv4_frames_desc, sccsum_ipv4_fill_desc and sccsum_spans_desc as they
 * stand, and sccsum_gather(d_desc, 2 * frames, dst) materialises the packed
 * wire frames.
 *
 * Input.  Datagram i of n is d_l4[d_off[i] .. + d_len[i]): L4 header + payload,
 * as ipv4::send receives `p`; d_dst[i] its destination (host order), d_proto[i]
 * its protocol, d_id[i] its identification (d_id NULL: 0, what the reference
 * writes, ip.cc:255).  opts: the source address (host order), the MTU
 * (68..65535) and SCCSUM_SEND_* flags.
 *
 * The cut.  needs_frag = len + 20 > mtu && !((proto == 6 && TSO) || (proto ==
 * 17 && UFO)).  A datagram that needs none is ONE frame with frag = 0 (an empty
 * datagram: a header-only frame).  Otherwise it is cut, in order, into pieces
 * of can_send = min(mtu - 20, remaining) bytes with
 * frag = (remaining_after > 0) << 13 | (offset / 8).  The division TRUNCATES,
 * exactly as the reference's does: with mtu - 20 not a multiple of 8 the
 * offsets are the reference's, not RFC 791's.
 *
 * The header of a frame: 0x45, 0, len = 20 + piece, id, frag, ttl 64, proto,
 * csum, src, dst (16- and 32-bit fields big-endian); csum = the RFC 1071
 * checksum of the 20 bytes with the field zero, computed from the fields, or 0
 * with SCCSUM_SEND_NO_IP_CSUM (tx_csum_ip_offload, ip.cc:271-273).
 *
 * Outputs, frame f (frames in datagram order, then piece order) of datagram i,
 * its piece at datagram offset o:
 *   d_hdr[20 f .. 20 f + 20)   the header
 *   d_out_off[f]               the frame's position in a PACKED layout: frames
 *                              back to back from 0
 *   d_out_len[f]               20 + piece
 *   d_desc[2f]                 {d_hdr + 20 f, d_out_off[f], 20}
 *   d_desc[2f + 1]             {d_l4 + d_off[i] + o, d_out_off[f] + 20, piece}
 *   d_first[f] = 2f            plus one closing entry after the last frame
 *   d_dgram_first[i]           datagram i's first frame; n + 1 entries
 *   d_status[i]  (required)    SCCSUM_ST_OK: emitted.  SCCSUM_ST_RANGE:
 *                              [off, off + len) is not inside [0, l4_bytes_len)
 *                              (the 64-bit test of sccsum_spans).
 *                              SCCSUM_ST_MALFORMED: len > 65515 (the reference's
 *                              uint16_t arithmetic would wrap).  Both bits when
 *                              both hold.  A refused datagram has no frame:
 *                              d_dgram_first[i + 1] == d_dgram_first[i].
 *   d_total[3]                 {frames all valid datagrams need, layout bytes
 *                              they need, datagrams emitted (the prefix)}
 *
 * Capacity, a prefix rule.  Datagram i is emitted only if over datagrams 0..i
 * the frames are <= max_frames (itself <= 2^31 - 1) and the layout bytes
 * <= max_out_bytes (itself <= 2^32 - 1: dst_off is 32-bit).  From the first
 * datagram that does not fit onward nothing is emitted: those datagrams' status
 * is 0 and their d_dgram_first entries (the closing one included) repeat the
 * number of frames emitted.  No per-frame array is written past what was
 * emitted (d_first: past its closing entry), so d_hdr holds 20 * max_frames
 * bytes, d_desc 2 * max_frames records, d_first max_frames + 1 entries,
 * d_out_off / d_out_len max_frames.  d_total reports the full need: a rerun
 * with those caps emits everything.
 *
 * SCCSUM_SEND_L4: d_l4sum[i] — what sccsum_spans returned for the datagram with
 * its pseudo-header seed and a zero field — is stored at UDP +6 (len >= 8) or
 * TCP +16 (len >= 20) of every emitted datagram before the cut; other
 * protocols and shorter datagrams are left alone.  It is the call's only write
 * into d_l4; d_l4sum must be NULL without the flag.
 *
 * Four small kernels on `stream` (count, scan, place, emit), one chain of plain
 * dependent launches: no allocation, no memset, no host synchronisation, no
 * atomic deciding a position — two runs give identical bytes; capturable.
 * d_workspace: sccsum_ipv4_send_workspace(n) bytes of device scratch, 16-byte
 * aligned.  Alignment: d_off, d_out_off, d_total and d_desc 8 bytes; d_len,
 * d_dst, d_first, d_out_len and d_dgram_first 4; d_id, d_l4sum 2; d_l4 and
 * d_hdr any (a 4-byte aligned d_hdr is stored as words).  SCCSUM_EINVAL before any device
 * work: mtu outside 68..65535, unknown flags, a NULL required pointer,
 * misalignment, a cap out of range, n > 2^32 - 1, d_l4sum without / the flag
 * without d_l4sum, a stream of another device.  n == 0 writes d_total,
 * d_dgram_first[0] (and d_first[0] when d_first is given) and is SCCSUM_OK;
 * the other arrays may then be NULL. */
#define SCCSUM_SEND_TSO        0x01u /* hw_features().tx_tso: a TCP datagram is never cut (ip.cc:105) */
#define SCCSUM_SEND_UFO        0x02u /* hw_features().tx_ufo: a UDP datagram is never cut (ip.cc:106) */
#define SCCSUM_SEND_NO_IP_CSUM 0x04u /* tx_csum_ip_offload: csum field left 0 (ip.cc:271-273) */
#define SCCSUM_SEND_L4         0x08u /* store d_l4sum[i] into datagram i's L4 field before the cut */

typedef struct sccsum_send_opts {
    uint32_t src_host; /* ipv4::_host_address, host order */
    uint32_t mtu;      /* hw_features().mtu, 68..65535 */
    uint32_t flags;
} sccsum_send_opts;

/* O(1) host arithmetic for one datagram (like sccsum_steer_dest): frames and
 * layout bytes ipv4::send makes of an L4 datagram of l4_len bytes; 0 frames
 * for l4_len > 65515 (SCCSUM_OK: the datagram would be refused) or bad opts
 * (SCCSUM_EINVAL, as for a NULL pointer). */
int sccsum_ipv4_send_plan(const sccsum_send_opts* opts, uint32_t l4_len, uint8_t proto,
                          uint32_t* nframes, uint64_t* out_bytes);

uint64_t sccsum_ipv4_send_workspace(uint64_t n);

int sccsum_ipv4_send(const sccsum_send_opts* opts,
                     void* d_l4, uint64_t l4_bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                     const uint32_t* d_dst, const uint8_t* d_proto, const uint16_t* d_id,
                     const uint16_t* d_l4sum, uint64_t n,
                     uint64_t max_frames, uint64_t max_out_bytes,
                     uint8_t* d_hdr, sccsum_gather_desc* d_desc, uint32_t* d_first,
                     uint64_t* d_out_off, uint32_t* d_out_len,
                     uint32_t* d_dgram_first, uint8_t* d_status, uint64_t* d_total,
                     void* d_workspace, void* stream);

/* ---- Rx reassembly: IPv4 fragments merged into fragment-list datagrams -----------
 * What ipv4::handle_received_packet does with an IP fragment (ip.cc:164-220),
 * ipv4::frag::merge / is_complete (ip.cc:412-437) and packet_merger::merge
 * (packet-util.hh:45-151), for a whole batch on the device.  As in Tx send, NO
 * payload byte moves: a reassembled datagram is one sccsum_gather_desc per
 * fragment, so the outputs are the arguments of sccsum_spans_desc (the L4
 * verify, tcp.hh:876-883: result 0) and sccsum_gather as they stand, and the
 * datagram hashes are what sccsum_steer_run(SCCSUM_STEER_HASH2CPU, ...) takes.
 * frag_timeout and frag_limit_mem stay host policy (the records' tag).
 *
 * sccsum_ipv4_frag_records: one sccsum_frag_rec per accepted frame of a frames
 * batch, a STABLE compaction in arrival order, and their count.
 *   d_bytes .. n     the batch, as sccsum_ipv4_frames took it
 *   d_status         what the frames call wrote for it (required)
 *   need / reject    frame i is accepted when (d_status[i] & need) == need &&
 *                    (d_status[i] & reject) == 0, as in sccsum_steer_run (8-bit
 *                    masks).  The documented default: need = SCCSUM_ST_OK |
 *                    SCCSUM_ST_IPFRAG, reject = SCCSUM_ST_MALFORMED |
 *                    SCCSUM_ST_RANGE — the fragments ip.cc:121-144 lets
 *                    through.  Whatever the masks say, a frame outside the
 *                    buffer, shorter than 20 bytes or than its IP total length,
 *                    with 4 * ihl past that length or offset + length past
 *                    65535 is skipped: its header is not trusted.
 *   host_address     host order; a frame with another destination is skipped
 *                    (ip.cc:159-162); 0 accepts any
 *   tag              copied into every record (the host's arrival stamp)
 *   d_rec            room for n records, 8-byte aligned; d_count: their number
 *   d_workspace      sccsum_ipv4_reasm_workspace(n) bytes suffice, 16-byte aligned
 * Records hold absolute addresses: the fragments of one datagram may lie in
 * different batches' buffers, which must stay where they are while a record
 * of theirs is pending.
 *
 * sccsum_ipv4_reasm: m records in arrival order (the caller puts the records an
 * earlier call left pending in front of the new batch's).  Key = ipv4_frag_id
 * {src, dst, id, proto} (ip.hh:243-256).  A key is PLAIN when, over its records
 * of this call in offset order, every len > 0, consecutive records do not
 * overlap (end_j <= offset_j+1) and at most one record has MF clear, the last
 * one.  For a plain key the reference's result does not depend on arrival
 * order: it completes exactly when the records tile [0, E) and the MF-clear
 * one is there, at the last of them to arrive.  Every record lands in exactly
 * one bucket, d_rec_state[i] (one byte per input record):
 *   SCCSUM_REASM_COMPLETE  its key is plain, starts at 0, every neighbour
 *                          touches and the MF-clear record is present
 *   SCCSUM_REASM_PENDING   its key is plain but not complete, or complete past
 *                          the capacity prefix (below)
 *   SCCSUM_REASM_HOST      its key is not plain (overlap, duplicate, empty
 *                          piece, data past the last fragment): the host replays
 *                          the key's records, in order, through the reference's
 *                          own merger, whose rules for them depend on arrival
 *                          order (packet-util.hh:55-86)
 * Records are grouped by a stable sort on sccsum_reasm_key_mix(key), 32 bits:
 * two distinct keys with one mix are both sent to the host bucket whole (never
 * merged with each other); no other plain key ever goes there.
 *
 * Per complete datagram d, in the order of the arrival index of its completing
 * record — the order ip.cc:180-189 delivers them in:
 *   d_dgram_first[d]   CSR index into d_desc; one closing entry after the last
 *   d_desc[...]        {frame + hdr_len, d_dgram_off[d] + offset, len} per
 *                      record, in offset order
 *   d_dgram_off[d]     64-bit position in a packed layout starting at 0
 *   d_dgram_len[d]     E, the datagram's bytes
 *   d_dgram_seed[d]    sccsum_pseudo_seed(src, dst, proto, E) for TCP / UDP, 0
 *                      for other protocols (as the frames calls treat ICMP)
 *   d_dgram_head[d]    index of the offset-0 record, whose IP header is the
 *                      one frag::merge keeps (ip.cc:416-418)
 *   d_dgram_last[d]    index of the completing record
 *   d_dgram_hash[d]    with `key` (host memory, key_len >= 4; both or neither):
 *                      the SCCSUM_RSS_REASSEMBLED hash of ip.cc:186-197 — src,
 *                      dst, then the first four datagram bytes when E holds
 *                      the TCP (20) / UDP (8) header
 * d_pending / d_host: the records of those buckets, copied, in arrival order.
 * d_total[4] = {datagrams, descriptors, pending, host} as emitted.  Every
 * array has room for m entries (d_dgram_first: m + 1).
 *
 * Capacity, Tx send's prefix rule: datagram d is emitted only while the packed
 * layout of datagrams 0..d is <= max_out_bytes (itself <= 2^32 - 1, the reach
 * of dst_off).  The records of the datagrams that do not fit are PENDING, so
 * the next call completes them; nothing is written past what was emitted.
 *
 * Plain dependent launches on `stream` (a key pass, six count / scan / scatter
 * passes of a stable radix sort, segmented scans and compactions): no
 * allocation, no memset, no host synchronisation, no atomic deciding a
 * position — two runs give identical bytes; capturable.  d_workspace:
 * sccsum_ipv4_reasm_workspace(m) bytes of device scratch, 16-byte aligned.
 * Alignment: records, d_desc, d_dgram_off and d_total 8 bytes, the 32-bit
 * arrays 4.  SCCSUM_EINVAL before any device work: a NULL required pointer,
 * misalignment, m or n > 2^31 - 1, max_out_bytes > 2^32 - 1, mask bits past
 * 0xFF, a key without d_dgram_hash or the reverse, key_len < 4, a stream of
 * another device.  m == 0 writes d_total and d_dgram_first[0] and is SCCSUM_OK;
 * the other arrays and the workspace may then be NULL.  n == 0 writes d_count. */
typedef struct sccsum_frag_rec {
    const void* frame;   /* the frame's IPv4 header, where it lies */
    uint32_t src, dst;   /* host order */
    uint16_t id;
    uint8_t  proto;
    uint8_t  mf;         /* 1 = MF set */
    uint16_t offset;     /* ip_hdr::offset(), ip.hh:402: uint16_t(frag << 3) */
    uint16_t hdr_len;    /* 4 * ihl */
    uint16_t len;        /* ip total length - 4 * ihl: the bytes merge() keeps */
    uint16_t reserved;   /* 0 */
    uint32_t tag;
} sccsum_frag_rec;

#define SCCSUM_REASM_COMPLETE 1
#define SCCSUM_REASM_PENDING  2
#define SCCSUM_REASM_HOST     3

typedef struct sccsum_reasm_out {
    sccsum_gather_desc* d_desc;   /* m */
    uint32_t* d_dgram_first;      /* m + 1 */
    uint64_t* d_dgram_off;        /* m */
    uint32_t* d_dgram_len;        /* m */
    uint32_t* d_dgram_seed;       /* m */
    uint32_t* d_dgram_head;       /* m */
    uint32_t* d_dgram_last;       /* m */
    uint32_t* d_dgram_hash;       /* m; NULL iff no key */
    sccsum_frag_rec* d_pending;   /* m */
    sccsum_frag_rec* d_host;      /* m */
    uint8_t* d_rec_state;         /* m */
    uint64_t* d_total;            /* 4 */
} sccsum_reasm_out;

int sccsum_ipv4_frag_records(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                             const uint8_t* d_status, uint32_t need, uint32_t reject, uint64_t n,
                             uint32_t host_address, uint32_t tag, sccsum_frag_rec* d_rec, uint32_t* d_count,
                             void* d_workspace, void* stream);

uint64_t sccsum_ipv4_reasm_workspace(uint64_t m);

int sccsum_ipv4_reasm(const sccsum_frag_rec* d_rec, uint64_t m, uint64_t max_out_bytes,
                      const uint8_t* key, uint32_t key_len, const sccsum_reasm_out* out,
                      void* d_workspace, void* stream);

/* The 32-bit mix of a key that sccsum_ipv4_reasm groups by (O(1), host). */
uint32_t sccsum_reasm_key_mix(uint32_t src_host, uint32_t dst_host, uint16_t id, uint8_t proto);

/* ---- Link layer: rx demux, ARP learn and lookup, tx Ethernet headers ----------------
 * The per-packet Ethernet steps of the reference around the IPv4 layer, for a
 * whole batch on the device (paths relative to the reference tree):
 *   interface::dispatch_packet   src/net/net.cc:324-357   sccsum_eth_rx
 *   _arp.learn(from, h.src_ip)   src/net/ip.cc:147-149, include/seastar/net/arp.hh:247-248
 *                                                          sccsum_arp_learn_records
 *   ipv4::get_l2_dst_address     ip.cc:231-242, arp.hh:214-216   \  sccsum_eth_send
 *   interface's packet provider  net.cc:266-284                  /
 * The ARP protocol itself (requests, replies, waiters, timeouts) stays on the
 * host.  No payload byte moves and no atomic decides a position: two runs give
 * identical bytes; plain dependent launches on `stream`, capturable.
 *
 * A MAC is a uint64_t whose low 48 bits are the six wire bytes as a big-endian
 * number (the first byte on the wire is the most significant); bits 48-63 are
 * 0.  IPv4 addresses are in host order.
 *
 * ARP table.  An immutable device copy of the stack's ARP table (like
 * sccsum_steer: a changed table is a new object, the old one destroyed once
 * its stream is synchronised).  entries[n] are host memory, n <= 2^20 (n == 0
 * allowed, entries may then be NULL); `pad` is ignored; any ip is a valid key,
 * 0 and 255.255.255.255 included (the reference seeds its table with broadcast
 * -> ff:ff:ff:ff:ff:ff, arp.hh:153: the caller adds that entry); when an ip
 * is given twice the later entry wins, as successive learn calls do.  Open
 * addressing with linear probing from sccsum_arp_table_slot(ip, bits), 16-byte
 * slots {ip, valid, mac} with the valid word apart from the key; 2^bits slots,
 * the smallest power of two >= max(16, 2 n), so every probe sequence meets an
 * empty slot.  create leaves the caller's current device alone; SCCSUM_EINVAL
 * for out == NULL, entries == NULL with n != 0, n > 2^20 or a MAC with bits
 * 48-63 set, before the device is looked at; SCCSUM_ENODEV for a device index
 * out of range.  sccsum_arp_table_lookup is host arithmetic on the object's
 * own copy: 1 on a hit (*mac written), 0 on a miss or a NULL argument.
 * sccsum_arp_table_slot is the home slot of a key in a table of 2^bits slots
 * (bits <= 31; UINT32_MAX past that), exported so that a test can build
 * colliding keys; sccsum_arp_table_bits is an object's bits (0 for NULL).
 *
 * sccsum_eth_rx: dispatch_packet for n wire frames d_bytes[d_off[i] .. +
 * d_len[i]).  protos[K] (HOST memory, 1 <= K <= 8, distinct) are the registered
 * eth_proto values in host order, e.g. {0x0800, 0x0806}.  Frame i is
 *   class k            d_len >= 14 and the big-endian 16 bits at +12 == protos[k]
 *   SCCSUM_ETH_UNKNOWN another eth_proto (_proto_map.find fails)
 *   SCCSUM_ETH_SHORT   d_len < 14 (get_header<eth_hdr> is null)
 *   SCCSUM_ETH_RANGE   [off, off + len) not inside [0, bytes_len), the 64-bit
 *                      test of sccsum_spans, made first: the frame is not read
 * and the last three are dropped.  As in the reference there is no VLAN
 * handling, no destination-MAC filter and no padding to a minimum length.
 *   d_class[n]    optional, arrival order: k or one of the three codes
 *   d_first[K+2]  bucket bases as sccsum_steer_run writes them: bucket k < K is
 *                 class k, bucket K the dropped frames, the last entry n
 *   d_order[n]    frame indices grouped by bucket, a STABLE partition (arrival
 *                 order inside a bucket)
 *   d_l3_off[n], d_l3_len[n], d_src_mac[n]   in grouped order (position j
 *                 describes frame d_order[j]): off + 14, len - 14 and the source
 *                 MAC for a classified frame (trim_front(14)); off, 0 and 0 for
 *                 a dropped one
 * so d_l3_off + d_first[k], d_l3_len + d_first[k], d_first[k+1] - d_first[k]
 * are a frames batch for sccsum_ipv4_frames* as they stand, and an ARP bucket
 * is the short index list the host copies back.  Three launches (count, scan,
 * scatter) over tiles of sccsum_eth_tile_packets() frames.  d_workspace:
 * sccsum_eth_rx_workspace(n) bytes, 16-byte aligned.  n <= 2^32 - 1.  n == 0
 * writes d_first (all 0) and is SCCSUM_OK; the frame arrays may then be NULL.
 *
 * sccsum_arp_learn_records: the learn candidates of ip.cc:147-149 among the n
 * frames of an IPv4 bucket, given as the frames batch above with the d_status
 * the frames call wrote for it and the bucket's slice of d_src_mac.  A STABLE
 * compaction in arrival order of sccsum_arp_rec {ip, index (into the bucket),
 * mac} into d_rec (room for n, 8-byte aligned) and their number in *d_count.
 * Frame i is kept when (d_status[i] & need) == need && (d_status[i] & reject)
 * == 0 (8-bit masks; the documented default need = SCCSUM_ST_OK, reject =
 * SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE is what ip.cc:121-144 lets through:
 * fragments pass, and so do packets for other destinations), its source
 * address src (header bytes 12-15) has ((src ^ host) & netmask) == 0 and src
 * != host, and `table` does not already map src to this MAC (a NULL table maps
 * nothing).  Whatever the masks say, a frame outside the buffer or shorter
 * than 20 bytes is skipped before its header is read.  The host applies the
 * records in order with the stack's own learn; in the steady state there are
 * none.  Repeats of one new (ip, mac) pair inside a batch are NOT removed.
 * d_workspace: sccsum_arp_learn_workspace(n) bytes, 16-byte aligned.  n <=
 * 2^31 - 1; n == 0 writes *d_count = 0.
 *
 * sccsum_eth_send: resolve the next hop of n datagrams and prepend the
 * Ethernet header to their frames, on fragment lists.  d_dst[n] are the
 * datagrams' destinations; d_dgram_first[n + 1] as sccsum_ipv4_send wrote it
 * (datagram i's frames are [d_dgram_first[i], d_dgram_first[i+1])), or NULL:
 * one frame per datagram (then F == n).  The F frames are fragment lists
 * d_desc, d_first[F + 1], d_off[F], d_len[F] as the *_desc calls take them,
 * with any number of descriptors per frame.  Run the checksum fills on those
 * lists BEFORE this call: an Ethernet descriptor in front of the IP header is
 * outside sccsum_ipv4_fill_desc's packet.
 *   Next hop of datagram i: d_dst[i] when ((dst ^ host) & netmask) == 0, gw
 * otherwise (netmask 0, the reference's initial value, puts every destination
 * on the link); it is RESOLVED when the table maps it.  A datagram without a
 * frame (refused by send, or past its prefix) is not looked up: status 0,
 * never listed.
 *   Input frame f of a resolved datagram becomes emitted frame f' (a stable
 * compaction over frames) at layout position o', positions packed back to
 * back from 0, each frame 14 bytes longer:
 *   d_eth[14 f' .. + 14)   dst MAC, src MAC = hw_address, eth_proto, big-endian
 *                          as hton(eth_hdr) leaves them
 *   d_desc_out             {d_eth + 14 f', o', 14}, then the frame's own
 *                          descriptors with dst_off - d_off[f] + o' + 14 (32-bit
 *                          arithmetic) and the same src and len; room for D + F
 *                          records, D the input's descriptor count (D + F <=
 *                          2^32 - 1)
 *   d_first_out[f']        CSR index into d_desc_out, one closing entry after
 *                          the last emitted frame (room for F + 1)
 *   d_off_out[f'] = o', d_len_out[f'] = d_len[f] + 14, d_frame_src[f'] = f
 * so sccsum_gather over d_desc_out yields packed wire frames, and the mapped
 * burst form takes the lists as they stand.
 *   d_status[n]       SCCSUM_ST_OK: resolved and emitted; SCCSUM_ST_NOARP:
 *                     unresolved, no frame emitted; 0: no frame, or past the
 *                     capacity prefix
 *   d_unresolved[n]   stable list of {datagram index, next hop} of the
 *                     SCCSUM_ST_NOARP datagrams: the host sends its ARP queries
 *                     and resubmits
 *   d_total[6]        {frames the resolved datagrams need, layout bytes they
 *                     need, datagrams taken (the prefix), unresolved in the
 *                     prefix}, then what was emitted: {frames, descriptors}
 *                     (the sizes of the per-frame arrays and of d_desc_out)
 * Capacity, Tx send's prefix rule: datagrams are taken in order while the
 * layout bytes of the resolved ones are <= max_out_bytes (itself <= 2^32 - 1);
 * from the first resolved datagram that does not fit onward nothing is emitted
 * or listed and the status is 0.  No array is written past what was emitted;
 * a rerun with the reported need emits everything.
 *   Four launches (count, scan, place, emit) over tiles of
 * sccsum_eth_tile_packets() datagrams.  d_workspace: sccsum_eth_send_workspace(n)
 * bytes, 16-byte aligned.  n <= 2^32 - 1, F <= 2^31 - 1.  n == 0 writes
 * d_total and d_first_out[0] and is SCCSUM_OK.
 *
 * Alignment: d_off, d_src_mac, records, descriptors, d_off_out, d_unresolved
 * and d_total 8 bytes; the 32-bit arrays 4; d_bytes and d_eth any.
 * SCCSUM_EINVAL before any device work, in every call: a NULL required
 * pointer, misalignment, K outside 1..8 or duplicate protos, a MAC with bits
 * 48-63 set, mask bits past 0xFF, n / F / max_out_bytes out of range, F != n
 * without d_dgram_first, a stream of another device than the current one (than
 * the table's, when a table is given). */
#define SCCSUM_ST_NOARP    0x20u /* eth_send: the next hop has no ARP entry, no frame emitted */
#define SCCSUM_ETH_UNKNOWN 0xFFu
#define SCCSUM_ETH_SHORT   0xFEu
#define SCCSUM_ETH_RANGE   0xFDu
#define SCCSUM_ETH_MAX_PROTOS 8
#define SCCSUM_ARP_MAX_ENTRIES (1u << 20)

typedef struct sccsum_arp_table sccsum_arp_table;
typedef struct sccsum_arp_entry {
    uint32_t ip;
    uint32_t pad;
    uint64_t mac;
} sccsum_arp_entry;

typedef struct sccsum_arp_rec {
    uint32_t ip;
    uint32_t index;
    uint64_t mac;
} sccsum_arp_rec;

typedef struct sccsum_eth_opts {
    uint64_t hw_address; /* interface::_hw_address */
    uint32_t host;       /* ipv4::_host_address */
    uint32_t netmask;    /* ipv4::_netmask */
    uint32_t gw;         /* ipv4::_gw_address */
    uint16_t eth_proto;  /* host order, 0x0800 for IPv4 */
} sccsum_eth_opts;

typedef struct sccsum_eth_unresolved {
    uint32_t dgram;
    uint32_t next_hop;
} sccsum_eth_unresolved;

int sccsum_arp_table_create(int device, const sccsum_arp_entry* entries, uint32_t n, sccsum_arp_table** out);
/* The same table without a device copy, for sccsum_arp_table_lookup alone (a
 * control plane that has no device at hand): the device calls refuse it with
 * SCCSUM_ENODEV, after their argument checks. */
int sccsum_arp_table_create_host(const sccsum_arp_entry* entries, uint32_t n, sccsum_arp_table** out);
int sccsum_arp_table_destroy(sccsum_arp_table* t);
int sccsum_arp_table_lookup(const sccsum_arp_table* t, uint32_t ip, uint64_t* mac);
uint32_t sccsum_arp_table_slot(uint32_t ip, uint32_t bits);
uint32_t sccsum_arp_table_bits(const sccsum_arp_table* t);

int sccsum_eth_tile_packets(void);
uint64_t sccsum_eth_rx_workspace(uint64_t n);
int sccsum_eth_rx(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len, uint64_t n,
                  const uint16_t* protos, uint32_t nprotos, uint8_t* d_class, uint32_t* d_first, uint32_t* d_order,
                  uint64_t* d_l3_off, uint32_t* d_l3_len, uint64_t* d_src_mac, void* d_workspace, void* stream);

uint64_t sccsum_arp_learn_workspace(uint64_t n);
int sccsum_arp_learn_records(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                             const uint8_t* d_status, uint32_t need, uint32_t reject, const uint64_t* d_src_mac,
                             uint64_t n, uint32_t host, uint32_t netmask, const sccsum_arp_table* table,
                             sccsum_arp_rec* d_rec, uint32_t* d_count, void* d_workspace, void* stream);

uint64_t sccsum_eth_send_workspace(uint64_t n);
int sccsum_eth_send(const sccsum_eth_opts* opts, const sccsum_arp_table* table, const uint32_t* d_dst,
                    const uint32_t* d_dgram_first, uint64_t n, const sccsum_gather_desc* d_desc,
                    const uint32_t* d_first, const uint64_t* d_off, const uint32_t* d_len, uint64_t nframes,
                    uint64_t max_out_bytes, uint8_t* d_eth, sccsum_gather_desc* d_desc_out, uint32_t* d_first_out,
                    uint64_t* d_off_out, uint32_t* d_len_out, uint32_t* d_frame_src, uint8_t* d_status,
                    sccsum_eth_unresolved* d_unresolved, uint64_t* d_total, void* d_workspace, void* stream);

/* ---- UDP layer: rx channel demux by port, tx headers in headroom ---------------------
 * The per-datagram UDP steps of the reference above the IPv4 layer, for a whole
 * batch on the device (paths relative to the reference tree):
 *   ipv4::handle_received_packet, its end   src/net/ip.cc:159-162, 222-227  \  sccsum_udp_rx,
 *   native_datagram, ipv4_udp::received     src/net/udp.cc:45-53, 164-173   /  sccsum_udp_rx_reasm
 *   ipv4_udp::send                          udp.cc:175-197                     sccsum_udp_send
 * No payload byte moves and no atomic decides a position: two runs give
 * identical bytes; plain dependent launches on `stream`, no allocation, no
 * memset, no host synchronisation; capturable.  Addresses and ports are in host
 * order.
 *
 * Port table.  An immutable device object (like sccsum_arp_table: a changed set
 * of channels is a new object, the old one destroyed once its stream is
 * synchronised).  ports[C] are HOST memory, distinct host-order ports, 0 <= C <=
 * SCCSUM_UDP_MAX_CHANNELS (252; ports may be NULL when C == 0); channel k is
 * ports[k], what ipv4_udp::_channels maps.  The device form is a 65 536-entry
 * byte table (port -> k, 0xFF unbound): one byte load per datagram.  create
 * leaves the caller's current device alone; SCCSUM_EINVAL for out == NULL,
 * ports == NULL with C != 0, C > 252 or a port given twice, before the device
 * is looked at; SCCSUM_ENODEV for a device index out of range.
 * sccsum_udp_ports_lookup is host arithmetic on the object's own copy: k, or -1
 * for an unbound port or a NULL table; sccsum_udp_ports_channels is C (0 for
 * NULL).  _create_host makes the same object without a device copy, for lookup
 * alone: the device calls refuse it with SCCSUM_ENODEV after their argument
 * checks.
 *
 * sccsum_udp_rx: the non-fragment frames of an IPv4 bucket.  The frames batch
 * (d_bytes, bytes_len, d_off, d_len, nbatch frames) as sccsum_ipv4_frames took
 * it, the d_status[nbatch] that call wrote, and 8-bit masks: a frame passes when
 * (d_status & need) == need && (d_status & reject) == 0.  The documented
 * default is need = SCCSUM_ST_OK, reject = SCCSUM_ST_MALFORMED |
 * SCCSUM_ST_RANGE | SCCSUM_ST_IPFRAG.  The reference does NOT verify the UDP
 * checksum on rx (udp.cc:164-173); a caller who wants it verified adds
 * SCCSUM_ST_L4_OK to need.  host_address: ipv4::_host_address, 0 accepts any
 * destination.  The call has n frames: frame j is batch frame d_index[j], or
 * batch frame j when d_index is NULL (then n <= nbatch) — a shard's slice of
 * sccsum_steer_run's grouped d_order goes in as it stands.
 *   Class of frame j (d_class[n], optional, in the call's order):
 *   SCCSUM_UDP_SKIP    not the UDP layer's.  Any of: d_index[j] >= nbatch; it
 *                      fails the masks; [off, off + len) is not inside [0,
 *                      bytes_len) (the 64-bit test of sccsum_spans, made before
 *                      the frame is read); it is shorter than 20 bytes or than
 *                      its IP total length, or 4 * ihl is past that length (the
 *                      header-trust rules of sccsum_ipv4_frag_records); MF is
 *                      set or the fragment offset is nonzero, read from the
 *                      header; dst != host_address; protocol != 17
 *   SCCSUM_UDP_SHORT   the L4 length ip_len - 4 * ihl < 8: get_header<udp_hdr>
 *                      is null there and the reference dereferences it; here
 *                      the frame is dropped
 *   SCCSUM_UDP_NOPORT  no channel on the big-endian 16 bits at L4 +2
 *                      (udp.cc:168-169: dropped silently, as in the reference)
 *   k                  the channel
 *   d_first[C + 2]  bucket bases as sccsum_eth_rx writes them: bucket k < C is
 *                   channel k, bucket C everything dropped, the last entry n
 *   d_order[n]      batch frame indices (d_index[j], or j) grouped by bucket, a
 *                   STABLE partition (the call's order inside a bucket)
 *   d_pay_off[n], d_pay_len[n], d_src[n], d_sport[n]   in grouped order: off + 4
 *                   ihl + 8, ip_len - 4 ihl - 8, the source address and the
 *                   source port of a frame with a channel; off, 0, 0, 0 for a
 *                   dropped one (0 for its off too when its index is out of
 *                   range).  The length is the trim to the IP total length
 *                   (ip.cc:225) and then everything behind the two headers:
 *                   udp_hdr::len is NOT consulted, as native_datagram does not
 *                   consult it
 * so d_pay_off + d_first[k], d_pay_len + d_first[k], d_first[k+1] - d_first[k]
 * are a spans batch as they stand.
 *   Queue room.  _queue.push drops a datagram when the channel's queue is full
 * (queue.hh:184-192; ipv4_udp::default_queue_size 1 024).  The partition is
 * stable, so the datagrams the reference accepts are the first min(count_k,
 * room_k) of bucket k: host arithmetic on C numbers, which the wrappers offer as
 * taken(k, room).  The device does not see room.
 *
 * sccsum_udp_rx_reasm: the same demux for the m datagrams sccsum_ipv4_reasm
 * emitted: its d_desc, d_dgram_first[m + 1], d_dgram_off, d_dgram_len,
 * d_dgram_head and the records d_rec[nrec] it took.  Source, destination and
 * protocol of datagram d come from d_rec[d_dgram_head[d]]; optional
 * d_l4_status[m] — what sccsum_spans_desc wrote for the L4 verify — with the
 * masks as above (NULL: the masks must be 0).  The eight header bytes are read
 * through the list, at layout positions d_dgram_off[d] + 0..7, byte-wise: the
 * list is in layout order and tiles the datagram, as reassembly writes it, so
 * the header may straddle up to eight descriptors; at most eight are walked and
 * none is read past d_dgram_first[d + 1].  Classes: SKIP (the masks, a head
 * index >= nrec, destination, protocol, a list whose first eight descriptors do
 * not hold the eight bytes), SHORT (E = d_dgram_len[d] < 8), NOPORT, k.
 * Outputs: d_class[m], d_first[C + 2], d_order[m] (datagram indices) and, in
 * grouped order, d_pay_len = E - 8, d_src, d_sport (0 for a dropped one).  The
 * payload is the datagram's layout bytes from +8, so sccsum_gather over
 * reassembly's own descriptors materialises it; no descriptor is rewritten.
 *
 * Both are three launches (count, scan, scatter; four past 31 channels) over
 * tiles of sccsum_eth_tile_packets() items, the two decodes sharing the
 * kernels: the count kernel decodes every item once and leaves 16 bytes of it
 * in the workspace for the scatter kernel, which reads no header.  d_workspace:
 * sccsum_udp_rx_workspace(n) / sccsum_udp_rx_reasm_workspace(m) bytes (16 per
 * item and the per-tile counts of 253 buckets), 16-byte aligned.  n, nbatch <= 2^32 - 1; m, nrec <= 2^31 - 1.  n == 0
 * (m == 0) writes d_first (all 0) and is SCCSUM_OK; the other arrays may then
 * be NULL.
 *
 * sccsum_udp_send: ipv4_udp::send's header for n payloads, written where
 * prepend_header puts it when the packet has headroom: payload i is
 * d_bytes[d_off[i] .. + d_len[i]) and the 8 bytes in front of it belong to the
 * call.  The caller's contract: no headroom overlaps another payload or
 * headroom.  This is the form that composes with sccsum_ipv4_send, which needs
 * header and payload contiguous.  d_dst[n], d_dport[n], d_sport[n]; opts: the
 * source address, the MTU (68..65535) and SCCSUM_UDP_* flags.  Per accepted
 * datagram the call writes at d_off - 8: sport, dport, len + 8 (big-endian),
 * checksum field 0, and
 *   d_l4_off = d_off - 8, d_l4_len = d_len + 8     sccsum_ipv4_send's d_off / d_len
 *   d_proto = 17 (optional array)                  its d_proto
 *   d_sum_len, d_seed                              with d_l4_off a spans batch whose
 *                                                  sccsum_spans results are the d_l4sum
 *                                                  sccsum_ipv4_send(SCCSUM_SEND_L4)
 *                                                  stores at UDP +6
 *   d_needs_csum (u8)                              offload_info::needs_csum
 * Full checksum (udp.cc:191-194): d_sum_len = d_l4_len, d_seed =
 * sccsum_pseudo_seed(src, dst, 17, d_l4_len); a result of 0 stays 0.  With
 * SCCSUM_UDP_CSUM_OFFLOAD (tx_csum_l4_offload) and no fragmentation needed
 * (udp.cc:188-190; needs_frag = d_l4_len + 20 > mtu && !SCCSUM_UDP_UFO,
 * ip.cc:100-111) the field must hold the folded pseudo-header sum, not
 * complemented: d_sum_len = 0 and d_seed = 0xFFFF ^ sccsum_pseudo_seed(...), so
 * the empty span's result is exactly that value, and d_needs_csum = 1.
 *   d_status[n] (required): SCCSUM_ST_OK; SCCSUM_ST_RANGE: d_off < 8 or [d_off
 * - 8, d_off + d_len) is not inside [0, bytes_len) (64-bit test);
 * SCCSUM_ST_MALFORMED: d_len > 65507, sccsum_ipv4_send's 65 515 less the
 * header; both bits when both hold.  A refused datagram writes nothing into
 * d_bytes and gets d_l4_off = UINT64_MAX, d_l4_len = d_sum_len = d_seed = 0,
 * d_needs_csum = 0, so sccsum_ipv4_send refuses it with SCCSUM_ST_RANGE and
 * emits no frame.  One elementwise kernel; n <= 2^32 - 1; n == 0 is SCCSUM_OK.
 *
 * Alignment: d_off, d_pay_off, d_dgram_off, d_l4_off, records and descriptors 8
 * bytes; the 32-bit arrays 4; the 16-bit arrays 2; d_bytes any.  SCCSUM_EINVAL
 * before any device work, in every call: a NULL required pointer,
 * misalignment, a NULL table, mask bits past 0xFF, masks without a status
 * array, n / nbatch / m / nrec out of range, n > nbatch without d_index, mtu
 * outside 68..65535, unknown flags, a stream of another device than the
 * table's (udp_send: than the current one). */
#define SCCSUM_UDP_NOPORT 0xFFu
#define SCCSUM_UDP_SHORT  0xFEu
#define SCCSUM_UDP_SKIP   0xFDu
#define SCCSUM_UDP_MAX_CHANNELS 252
#define SCCSUM_UDP_CSUM_OFFLOAD 0x01u /* hw_features().tx_csum_l4_offload (udp.cc:188) */
#define SCCSUM_UDP_UFO          0x02u /* hw_features().tx_ufo: a UDP datagram is never cut (ip.cc:106) */

typedef struct sccsum_udp_ports sccsum_udp_ports;
typedef struct sccsum_udp_opts {
    uint32_t src_host; /* ipv4::_host_address, host order */
    uint32_t mtu;      /* hw_features().mtu, 68..65535 */
    uint32_t flags;
} sccsum_udp_opts;

int sccsum_udp_ports_create(int device, const uint16_t* ports, uint32_t channels, sccsum_udp_ports** out);
int sccsum_udp_ports_create_host(const uint16_t* ports, uint32_t channels, sccsum_udp_ports** out);
int sccsum_udp_ports_destroy(sccsum_udp_ports* t);
int sccsum_udp_ports_lookup(const sccsum_udp_ports* t, uint16_t port);
uint32_t sccsum_udp_ports_channels(const sccsum_udp_ports* t);

uint64_t sccsum_udp_rx_workspace(uint64_t n);
int sccsum_udp_rx(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                  uint64_t nbatch, const uint8_t* d_status, uint32_t need, uint32_t reject, uint32_t host_address,
                  const sccsum_udp_ports* ports, const uint32_t* d_index, uint64_t n, uint8_t* d_class,
                  uint32_t* d_first, uint32_t* d_order, uint64_t* d_pay_off, uint32_t* d_pay_len, uint32_t* d_src,
                  uint16_t* d_sport, void* d_workspace, void* stream);

uint64_t sccsum_udp_rx_reasm_workspace(uint64_t m);
int sccsum_udp_rx_reasm(const sccsum_gather_desc* d_desc, const uint32_t* d_dgram_first, const uint64_t* d_dgram_off,
                        const uint32_t* d_dgram_len, const uint32_t* d_dgram_head, uint64_t m,
                        const sccsum_frag_rec* d_rec, uint64_t nrec, const uint8_t* d_l4_status, uint32_t need,
                        uint32_t reject, uint32_t host_address, const sccsum_udp_ports* ports, uint8_t* d_class,
                        uint32_t* d_first, uint32_t* d_order, uint32_t* d_pay_len, uint32_t* d_src, uint16_t* d_sport,
                        void* d_workspace, void* stream);

int sccsum_udp_send(const sccsum_udp_opts* opts, void* d_bytes, uint64_t bytes_len, const uint64_t* d_off,
                    const uint32_t* d_len, const uint32_t* d_dst, const uint16_t* d_dport, const uint16_t* d_sport,
                    uint64_t n, uint64_t* d_l4_off, uint32_t* d_l4_len, uint32_t* d_sum_len, uint32_t* d_seed,
                    uint8_t* d_proto, uint8_t* d_needs_csum, uint8_t* d_status, void* stream);

/* ---- TCP layer: rx demux by connection, resets, tx headers in headroom ----------------
 * The stateless per-segment TCP steps of the reference above the IPv4 layer,
 * for a whole batch on the device (paths relative to the reference tree):
 *   ipv4::handle_received_packet, its end   src/net/ip.cc:159-162, 222-227        \
 *   tcp::received, before any tcb is touched  include/seastar/net/tcp.hh:865-942   > sccsum_tcp_rx
 *   tcp::respond_with_reset                 tcp.hh:981-1023                        /
 *   tcp_hdr::read / write                   tcp.hh:246-282
 *   tcb::output_one, its header             tcp.hh:1620-1698                         sccsum_tcp_send
 * The state machine (input_handle_*_state, timers, retransmit, option
 * negotiation) stays on the host; it runs per connection over a contiguous slice
 * of parsed records.  No payload byte moves and no atomic decides a position:
 * two runs give identical bytes; plain dependent launches on `stream`, no
 * allocation, no memset, no host synchronisation; capturable.  Addresses and
 * ports are in host order.
 *
 * Connection table.  An immutable device object (like sccsum_arp_table: a
 * changed set of connections is a new object, the old one destroyed once its
 * stream is synchronised).  conns[nconns] are HOST memory, nconns <=
 * SCCSUM_TCP_MAX_CONNS (2^20; conns may be NULL when nconns == 0); connection c
 * is conns[c], what tcp::_tcbs maps for that connid whatever its state: a
 * SYN_SENT tcb is an entry like any other, the split of tcp.hh:932-940 is the
 * host's, per connection.  listen[nlisten] are the distinct ports of
 * tcp::_listening, nlisten <= 65 536.  The device form of the connections is
 * open addressing with linear probing over 2^bits 16-byte slots {local_ip,
 * foreign_ip, local_port << 16 | foreign_port, c + 1} (0 in the last word:
 * empty), 2^bits the smallest power of two >= max(16, 2 nconns): a probe is one
 * 16-byte load, and any 96-bit key is valid, all zeros included.  The home slot
 * is an fmix32-style mix of the three key words, which sccsum_tcp_conns_slot
 * exports (its low `bits` bits).  The listening ports are a 65 536-entry byte
 * table.  create leaves the caller's current device alone; SCCSUM_EINVAL for
 * out == NULL, a NULL array with a nonzero count, a count past its limit, a
 * connid given twice (a map has no duplicate keys) or a port given twice, before
 * the device is looked at; SCCSUM_ENODEV for a device index out of range.
 * _lookup (the index, or -1; -1 for a NULL table) and _listening (1 / 0) are
 * host arithmetic on the object's own copy; _bits and _count are 0 for NULL.
 * _create_host makes the same object without a device copy, for lookup alone:
 * the device calls refuse it with SCCSUM_ENODEV after their argument checks.
 *
 * sccsum_tcp_rx: the non-fragment frames of an IPv4 bucket; the input is exactly
 * what sccsum_udp_rx takes (the frames batch, d_status[nbatch], the masks need /
 * reject, host_address with 0 accepting any destination, d_index[n] or NULL with
 * n <= nbatch).  The documented default is need = SCCSUM_ST_OK | SCCSUM_ST_L4_OK,
 * reject = SCCSUM_ST_MALFORMED | SCCSUM_ST_RANGE | SCCSUM_ST_IPFRAG: unlike UDP
 * the reference does verify the TCP checksum on rx (tcp.hh:876-883); a caller
 * with rx_csum_offload drops SCCSUM_ST_L4_OK from need.
 *   Class of frame j (d_class[n], optional, in the call's order), with E =
 * ip_len - 4 ihl (the L4 length after the trims of ip.cc:134-136, 225) and H = 4
 * * (byte 12 of the L4 >> 4), decided in this order:
 *   SCCSUM_TCP_SKIP    sccsum_udp_rx's SKIP rules word for word, with protocol != 6
 *   SCCSUM_TCP_SHORT   E < 20 (tcp.hh:866-869) or H < 20 (tcp.hh:871-874): both
 *                      silent drops in the reference
 *   SCCSUM_TCP_CONN    the connid {dst, src, dport, sport} (tcp.hh:885) is in the
 *                      table, and H <= E
 *   SCCSUM_TCP_LISTEN  not in the table, dport is listening, and H <= E
 *   SCCSUM_TCP_SHORT   in the table or listening, and H > E: the options are not
 *                      inside the segment.  The reference's trim_front(H) /
 *                      get_header(0, H) asserts or yields null there
 *                      (tcp.hh:1117-1119, 1216); here the frame is dropped
 *   SCCSUM_TCP_RESET   no connection, no listener, RST clear: respond_with_reset
 *                      (tcp.hh:898).  H > E does not matter: the reference reads
 *                      only the twenty fixed bytes
 *   SCCSUM_TCP_NOCONN  no connection, no listener, RST set: discarded (tcp.hh:983-985)
 * Everything order-dependent — listener->full(), a new tcb that a later segment
 * of the same batch would find, the RST / ACK / SYN triage of tcp.hh:900-929 —
 * lands in the LISTEN bucket in arrival order, for the host to walk with its
 * real _tcbs: every segment of a connid that is not in the table but whose port
 * listens reaches the host in arrival order, so no outcome depends on the
 * device's view being stale.
 *   d_first[5]   bucket bases: bucket 0 CONN, 1 LISTEN, 2 RESET, 3 everything
 *                dropped (NOCONN, SHORT, SKIP); the last entry n
 *   d_order[n]   batch frame indices grouped by bucket.  Inside bucket 0 by
 *                ascending connection index, the call's order inside a
 *                connection (a STABLE sort: a connection's segments reach its tcb
 *                in arrival order); buckets 1 to 3 are stable partitions
 *   d_seg[n]     one sccsum_tcp_seg per position of d_order, 8-byte aligned.
 *                Classes CONN, LISTEN, RESET, NOCONN: pay_off = off + 4 ihl + H
 *                (the options are the H - 20 bytes before it), pay_len = E - H
 *                (seg_len of tcp.hh:1221 before SYN / FIN are counted; 0 where H
 *                > E), the twenty fixed bytes parsed; conn the connection index
 *                in bucket 0, UINT32_MAX elsewhere.  SKIP and SHORT: pay_off =
 *                off (0 when the index is out of range), conn = UINT32_MAX, all
 *                other fields 0
 *   d_src[n]     the source addresses in grouped order, 0 for SKIP and SHORT
 *   d_run_conn[R], d_run_first[R + 1]   the runs of bucket 0: run r is connection
 *                d_run_conn[r], positions d_run_first[r] .. d_run_first[r + 1]
 *                of d_order / d_seg (the closing entry is d_first[1]); each array
 *                has room for min(n, nconns) + 1 entries.  A connection's slice
 *                of d_seg is d_seg + d_run_first[r], and its pay_off / pay_len
 *                are a spans batch
 *   d_rst, d_rst_dst   the r-th segment of bucket 2 is answered at d_rst[20 r ..
 *                + 20) as respond_with_reset writes it: ports swapped; seq =
 *                SEG.ACK when ACK is set, else 0; with SYN set ack = SEG.SEQ + 1
 *                and the ACK flag; RST set, data_offset 5, window and urgent 0.
 *                The checksum field is the full checksum (pseudo-header {local =
 *                dst, foreign = src, 6, 20} plus the twenty bytes), or with
 *                `flags` = SCCSUM_TCP_CSUM_OFFLOAD the folded pseudo-header sum,
 *                not complemented.  d_rst_dst[r] is the foreign address.  d_rst
 *                (room for 20 n bytes, 4-byte aligned), offsets 20 r, lengths 20,
 *                protocol 6 and d_rst_dst are an L4 batch for sccsum_ipv4_send as
 *                they stand, without SCCSUM_SEND_L4.  send_packet_without_tcb
 *                drops what does not fit _queue_space (tcp.hh:946-953): the list
 *                is stable, so that is the first min(count, space / 20) entries,
 *                host arithmetic the wrappers offer as taken(space)
 *   d_total[4]   {R, resets, 0, 0}, 8-byte aligned
 * The decode kernel reads every frame once and leaves its record and a sort key
 * in the workspace; the key is the connection index for bucket 0 and nconns + 0
 * / 1 / 2 for buckets 1 to 3, so one stable LSD radix sort in 8-bit digits
 * yields the grouped order and the bucket bases: one pass up to 253 connections,
 * two up to 65 533, three beyond.  d_workspace: sccsum_tcp_rx_workspace(n,
 * nconns) bytes, 16-byte aligned.  n, nbatch <= 2^32 - 1.  n == 0 writes d_first
 * and d_total (all 0) and d_run_first[0], and is SCCSUM_OK; the other arrays may
 * then be NULL.
 *
 * sccsum_tcp_send: output_one's header for n segments.  Payload i is
 * d_bytes[d_off[i] .. + d_len[i]) and the d_out[i].hdr_len bytes in front of it
 * (20..60, a multiple of 4) belong to the call; the caller has already written
 * the option bytes at [d_off - hdr_len + 20, d_off) (tcp_option::fill, SYN
 * segments only).  The call writes the twenty fixed bytes at d_off - hdr_len as
 * tcp_hdr::write does: ports, seq, ack, data_offset = hdr_len / 4, the flags
 * byte as given, window, checksum 0, urgent 0, and
 *   d_l4_off = d_off - hdr_len, d_l4_len = d_len + hdr_len, d_proto = 6 (optional)
 *   d_sum_len, d_seed   the spans batch whose sccsum_spans results
 *                       sccsum_ipv4_send(SCCSUM_SEND_L4) stores at TCP +16
 *   d_needs_csum (u8), d_tso_seg (u16)   offload_info::needs_csum, tso_seg_size
 * The three forms of tcp.hh:1662-1694.  Full: d_sum_len = d_l4_len, d_seed =
 * sccsum_pseudo_seed(src, dst, 6, d_l4_len).  SCCSUM_TCP_CSUM_OFFLOAD: d_sum_len
 * = 0, d_seed = 0xFFFF ^ sccsum_pseudo_seed(src, dst, 6, d_l4_len), so the empty
 * span's result is the folded pseudo-header sum, and d_needs_csum = 1.
 * SCCSUM_TCP_CSUM_OFFLOAD | SCCSUM_TCP_TSO with d_len > mss: the same with the
 * pseudo-header's length 0, and d_tso_seg = mss; d_tso_seg = 0 otherwise
 * (SCCSUM_TCP_TSO without the offload flag changes nothing, as in the reference).
 *   d_status[n] (required): SCCSUM_ST_OK; SCCSUM_ST_RANGE: d_off < hdr_len (as
 * given) or [d_off, d_off + d_len) is not inside [0, bytes_len) (64-bit test);
 * SCCSUM_ST_MALFORMED: hdr_len outside 20..60 or not a multiple of 4, d_len +
 * hdr_len > 65 515, SCCSUM_TCP_TSO with mss == 0; both bits when both hold.  A
 * refused segment writes nothing into d_bytes and gets d_l4_off = UINT64_MAX,
 * d_l4_len = d_sum_len = d_seed = 0, d_tso_seg = 0, d_needs_csum = 0; d_proto,
 * where given, is 6 for every segment, refused ones included (as
 * sccsum_udp_send writes its 17): sccsum_ipv4_send refuses the segment by its
 * offset, whatever the protocol says.  opts: the
 * source address, the MTU (68..65535) and SCCSUM_TCP_* flags.  One elementwise
 * kernel; n <= 2^32 - 1; n == 0 is SCCSUM_OK.
 *
 * No output array may overlap another output array, an input or the workspace:
 * the launches of one call read what earlier ones wrote (sccsum_tcp_rx's reset
 * kernel reads d_seg, d_first and the workspace; the run kernels read d_first),
 * so an aliased array gives wrong results without an error.  The call does not
 * check this.
 *
 * Alignment: d_off, d_seg, d_l4_off, d_total 8 bytes; the 32-bit arrays, d_rst
 * and d_out 4; the 16-bit arrays 2; d_bytes any.  SCCSUM_EINVAL before any
 * device work, in every call: a NULL required pointer, misalignment, a NULL
 * table, mask bits past 0xFF, n / nbatch out of range, n > nbatch without
 * d_index, mtu outside 68..65535, unknown flags, a stream of another device than
 * the table's (tcp_send: than the current one). */
#define SCCSUM_TCP_CONN   0x00u
#define SCCSUM_TCP_LISTEN 0x01u
#define SCCSUM_TCP_RESET  0x02u
#define SCCSUM_TCP_NOCONN 0x03u
#define SCCSUM_TCP_SHORT  0xFEu
#define SCCSUM_TCP_SKIP   0xFDu
#define SCCSUM_TCP_MAX_CONNS (1u << 20)
#define SCCSUM_TCP_CSUM_OFFLOAD 0x01u /* hw_features().tx_csum_l4_offload (tcp.hh:1008, 1662) */
#define SCCSUM_TCP_TSO          0x02u /* hw_features().tx_tso (tcp.hh:1674) */

typedef struct sccsum_tcp_conns sccsum_tcp_conns;
typedef struct sccsum_tcp_conn {
    uint32_t local_ip, foreign_ip;
    uint16_t local_port, foreign_port;
} sccsum_tcp_conn;
typedef struct sccsum_tcp_seg {
    uint64_t pay_off; /* off + 4 ihl + H: the bytes behind the header */
    uint32_t pay_len; /* E - H */
    uint32_t seq, ack; /* host order */
    uint32_t conn;    /* connection index; UINT32_MAX outside bucket 0 */
    uint16_t window, sport, dport;
    uint8_t flags;    /* byte 13 of the header as it stands: FIN 1, SYN 2, RST 4, PSH 8, ACK 16, URG 32 */
    uint8_t hdr_len;  /* H */
} sccsum_tcp_seg;
typedef struct sccsum_tcp_out {
    uint32_t dst, seq, ack;
    uint16_t sport, dport, window;
    uint8_t flags, hdr_len;
    uint32_t mss;     /* _snd.mss: consulted with SCCSUM_TCP_TSO */
} sccsum_tcp_out;
typedef struct sccsum_tcp_opts {
    uint32_t src_host; /* ipv4::_host_address, host order */
    uint32_t mtu;      /* hw_features().mtu, 68..65535 */
    uint32_t flags;
} sccsum_tcp_opts;

int sccsum_tcp_conns_create(int device, const sccsum_tcp_conn* conns, uint32_t nconns, const uint16_t* listen,
                            uint32_t nlisten, sccsum_tcp_conns** out);
int sccsum_tcp_conns_create_host(const sccsum_tcp_conn* conns, uint32_t nconns, const uint16_t* listen,
                                 uint32_t nlisten, sccsum_tcp_conns** out);
int sccsum_tcp_conns_destroy(sccsum_tcp_conns* t);
int64_t sccsum_tcp_conns_lookup(const sccsum_tcp_conns* t, uint32_t local_ip, uint32_t foreign_ip, uint16_t local_port,
                                uint16_t foreign_port);
int sccsum_tcp_conns_listening(const sccsum_tcp_conns* t, uint16_t port);
uint32_t sccsum_tcp_conns_slot(uint32_t local_ip, uint32_t foreign_ip, uint16_t local_port, uint16_t foreign_port,
                               uint32_t bits);
uint32_t sccsum_tcp_conns_bits(const sccsum_tcp_conns* t);
uint32_t sccsum_tcp_conns_count(const sccsum_tcp_conns* t);

uint64_t sccsum_tcp_rx_workspace(uint64_t n, uint32_t nconns);
int sccsum_tcp_rx(const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off, const uint32_t* d_len,
                  uint64_t nbatch, const uint8_t* d_status, uint32_t need, uint32_t reject, uint32_t host_address,
                  const sccsum_tcp_conns* conns, const uint32_t* d_index, uint64_t n, uint32_t flags, uint8_t* d_class,
                  uint32_t* d_first, uint32_t* d_order, sccsum_tcp_seg* d_seg, uint32_t* d_src, uint32_t* d_run_conn,
                  uint32_t* d_run_first, void* d_rst, uint32_t* d_rst_dst, uint64_t* d_total, void* d_workspace,
                  void* stream);

int sccsum_tcp_send(const sccsum_tcp_opts* opts, void* d_bytes, uint64_t bytes_len, const uint64_t* d_off,
                    const uint32_t* d_len, const sccsum_tcp_out* d_out, uint64_t n, uint64_t* d_l4_off,
                    uint32_t* d_l4_len, uint32_t* d_sum_len, uint32_t* d_seed, uint16_t* d_tso_seg, uint8_t* d_proto,
                    uint8_t* d_needs_csum, uint8_t* d_status, void* stream);

/* ---- TCP receive fast path: the in-sequence data of every connection's run ------------
 * Van Jacobson's header prediction for a batch.  Of tcb::input_handle_other_state
 * (include/seastar/net/tcp.hh:1215-1575) almost every segment of a bulk receiver
 * takes one path: acceptable (tcp.hh:1058-1076), exactly at RCV.NXT, with data,
 * no control flag besides ACK (PSH allowed), acknowledging nothing new.  There the
 * reference does only step 4.7 (tcp.hh:1497-1521): the text is appended to
 * _rcv.data, _rcv.next advances, _rcv.window is recomputed (tcp.hh:424-427) and
 * should_send_ack (tcp.hh:1845-1872) is stepped.  No send-side state moves, so
 * segment i's outcome depends only on sums over the segments before it.
 *
 * sccsum_tcp_rx_data takes the leading stretch of such segments of every run of
 * sccsum_tcp_rx's bucket 0 and leaves the host one record per run, plus the rest
 * of any run that left the straight path: d_seg[d_run_first[r] + taken ..
 * d_run_first[r + 1]), which the host walks with its real tcb as before, starting
 * from the state in the run record.  Whatever the device does not take reaches
 * the host whole and in order, so no outcome depends on the device.
 *
 * Inputs: d_seg, d_first, d_run_conn, d_run_first, d_total (here d_rx_total) as
 * sccsum_tcp_rx left them on the device, and its n (an upper bound that sizes the
 * launches; bucket 0 ends at d_first[1], R is d_rx_total[0]: no host
 * synchronisation, capturable).  d_bytes is the frames' buffer and is never read:
 * it only forms src = d_bytes + pay_off.  d_rcv[nconns], indexed by connection
 * index, 16-byte aligned, is the host's view of each tcb:
 *   next, window   _rcv.next, _rcv.window as it stands (tcp.hh:1059-1075)
 *   room           max_receive_buf_size - data_size, 0 if data_size is larger (tcp.hh:425)
 *   cap            get_default_receive_window_size() (tcp.hh:418-422)
 *   snd_una, mss   _snd.unacknowledged, _rcv.mss
 *   flags          SCCSUM_TCP_RCV_ELIGIBLE: set by the host only for a tcb in
 *                  ESTABLISHED with an empty _rcv.out_of_order, _snd.window > 0 and
 *                  _snd.unacknowledged <= _snd.next; _NR_FULL:
 *                  _nr_full_seg_received (0 or 1); _ACK_ARMED: _delayed_ack.armed()
 * room and cap above 2^30 are read as 2^30.
 *
 * The rule, per run r of connection c = d_run_conn[r], with a running next,
 * window, room that start from d_rcv[c]: segment i is taken iff every earlier one
 * was and none of these holds, tested in this order; the first that holds is the
 * run's `stop`:
 *   _STOP_INELIGIBLE  ELIGIBLE clear
 *   _STOP_WINDOW      pay_len > 0 and window == 0          (tcp.hh:1072-1075)
 *   _STOP_SEQ         seq != next                          (tcp.hh:1231-1245)
 *   _STOP_FLAGS       (flags & 0x37) != 0x10: FIN, SYN, RST or URG, or no ACK
 *   _STOP_ACK         ack != snd_una                       (tcp.hh:1336-1444)
 *   _STOP_EMPTY       pay_len == 0: a pure ACK             (tcp.hh:1401)
 *   _STOP_CAPACITY    below
 *   _STOP_END (0)     the run is exhausted
 * A taken segment: next += pay_len (mod 2^32); room = room >= pay_len ? room -
 * pay_len : 0; window = min(room, cap); one step of should_send_ack(pay_len) with
 * the connection's mss (its argument is a uint16_t: pay_len's low 16 bits), and
 * when that returns true the closing clear_delayed_ack(); output() (tcp.hh:1570-
 * 1574): the timer is off and _ACK_NOW is set.  Sums over a run are 64-bit: the
 * comparison against room does not wrap.
 *
 * d_run[R] (room for min(n, nconns) + 1, 8-byte aligned): taken, bytes (their
 * text); next, window, room after them (window as given when taken == 0);
 * desc_first, the exclusive scan of taken, and dst_off, that of bytes; flags:
 * _NR_FULL and _ACK_ARMED after them, _ACK_REARMED: arm(200 ms) was called during
 * them (when _ACK_ARMED is set too, the deadline is now + 200 ms, else the timer
 * the host holds is still the one that runs), _ACK_NOW: output() was called at
 * least once; stop.
 * d_desc[n] (8-byte aligned): taken segment k of run r is d_desc[desc_first + k] =
 * {d_bytes + pay_off, its dst_off, pay_len}, grouped by run in arrival order: one
 * sccsum_gather(d_desc, d_total[0], buf) packs every connection's new in-order
 * bytes, run r's at [dst_off, dst_off + bytes).  Entries from d_total[0] on are
 * not written.
 * Capacity (sccsum_ipv4_send's prefix rule): runs are taken in run order while the
 * packed text of runs 0..r is <= max_bytes (<= 2^32 - 1).  From the first run that
 * does not fit onward taken = 0, stop = _STOP_CAPACITY and the state is as given.
 * d_total[4] = {sum of taken as emitted, sum of bytes as emitted, the bytes needed
 * without the capacity, 0}, 8-byte aligned.
 *
 * Plain dependent launches on `stream` (tile, carry, tile, carry, place, and one
 * over the runs), no allocation, no memset, no atomic; two runs give identical
 * bytes.  d_workspace: sccsum_tcp_rx_data_workspace(n, nconns) bytes, 16-byte
 * aligned.  No output may overlap another array of the call.  SCCSUM_EINVAL
 * before any device work: a NULL required pointer (d_total and the workspace
 * always; with n != 0 every other one but d_bytes, and d_rcv unless nconns == 0),
 * misalignment (d_rcv and the workspace 16; d_seg, d_desc, d_total, d_rx_total and
 * d_run 8; the 32-bit arrays 4), n > 2^32 - 1, nconns > SCCSUM_TCP_MAX_CONNS,
 * max_bytes > 2^32 - 1, a stream of another device than the current one.  n == 0
 * writes d_total (all 0) and is SCCSUM_OK. */
#define SCCSUM_TCP_RCV_ELIGIBLE    0x01u
#define SCCSUM_TCP_RCV_NR_FULL     0x02u
#define SCCSUM_TCP_RCV_ACK_ARMED   0x04u
#define SCCSUM_TCP_RCV_ACK_REARMED 0x08u
#define SCCSUM_TCP_RCV_ACK_NOW     0x10u
#define SCCSUM_TCP_STOP_END        0u
#define SCCSUM_TCP_STOP_INELIGIBLE 1u
#define SCCSUM_TCP_STOP_WINDOW     2u
#define SCCSUM_TCP_STOP_SEQ        3u
#define SCCSUM_TCP_STOP_FLAGS      4u
#define SCCSUM_TCP_STOP_ACK        5u
#define SCCSUM_TCP_STOP_EMPTY      6u
#define SCCSUM_TCP_STOP_CAPACITY   7u

typedef struct sccsum_tcp_rcv {
    uint32_t next, window, room, cap, snd_una;
    uint16_t mss;
    uint8_t flags; /* SCCSUM_TCP_RCV_ELIGIBLE | _NR_FULL | _ACK_ARMED */
    uint8_t pad;
    uint32_t reserved[2]; /* ignored */
} sccsum_tcp_rcv;
typedef struct sccsum_tcp_rcv_run {
    uint32_t taken, bytes;
    uint32_t next, window, room;
    uint32_t desc_first, dst_off;
    uint8_t flags; /* SCCSUM_TCP_RCV_NR_FULL | _ACK_ARMED | _ACK_REARMED | _ACK_NOW */
    uint8_t stop;  /* SCCSUM_TCP_STOP_* */
    uint16_t pad;
} sccsum_tcp_rcv_run;

uint64_t sccsum_tcp_rx_data_workspace(uint64_t n, uint32_t nconns);
int sccsum_tcp_rx_data(const void* d_bytes, const sccsum_tcp_seg* d_seg, const uint32_t* d_first,
                       const uint32_t* d_run_conn, const uint32_t* d_run_first, const uint64_t* d_rx_total, uint64_t n,
                       const sccsum_tcp_rcv* d_rcv, uint32_t nconns, uint64_t max_bytes, sccsum_tcp_rcv_run* d_run,
                       sccsum_gather_desc* d_desc, uint64_t* d_total, void* d_workspace, void* stream);

/* ---- TCP transmit fast path: every polled connection's unsent queue cut into segments ----
 * The tx recipe of sccsum_tcp_send starts from payloads and one sccsum_tcp_out
 * per segment: the host has cut every segment and written its seq.  That cut is
 * tcb::get_packet's continuation (include/seastar/net/tcp.hh:2089-2111) calling
 * can_send() (tcp.hh:515-549), get_transmit_packet() (tcp.hh:1578-1606) and
 * output_one()'s sequence bookkeeping (tcp.hh:1635-1645) once per segment.  For a
 * tcb in ESTABLISHED or CLOSE_WAIT (ACK on, no SYN, no FIN: tcp.hh:631-640) with
 * _snd.dupacks == 0, _snd.window_probe false and an empty _packetq the whole
 * chain is a closed form of the state and the queue's length, and
 * sccsum_tcp_tx_data evaluates it for a batch: one record per connection going
 * in, one per connection and one per segment coming out.  Every other tcb
 * (dupacks 1 or 2: limited transmit, which mutates _snd.limited_transfer;
 * dupacks >= 3; window probes; SYN and closing states) is left untouched for the
 * host's own walk, so no outcome depends on the device.
 *
 * d_snd[nconns] (48 bytes each, 16-byte aligned), one per polled connection:
 *   dst, sport, dport       the foreign address, the local and the foreign port
 *   next, una, window, cwnd, mss    of _snd (unacknowledged as una)
 *   rcv_next                _rcv.next
 *   wnd                     the 16-bit header window, _rcv.window >> _rcv.window_scale
 *   flags                   SCCSUM_TCP_SND_ELIGIBLE: set by the host only under the
 *                           four conditions above; _RTX_ARMED: _retransmit.armed()
 * The unsent queues as a CSR: connection c's buffers are j in [d_buf_first[c],
 * d_buf_first[c + 1]) (nconns + 1 non-decreasing entries from 0 to at most nbuf),
 * buffer j the d_buf_len[j] bytes at the 64-bit address d_buf_src[j] (device
 * memory, or pinned / registered host memory, as sccsum_gather takes; never read
 * here).  A buffer of no bytes contributes no descriptor (the reference appends
 * an empty fragment, which changes nothing on the wire).  U, _snd.unsent_len, is
 * the 64-bit sum of the connection's lengths; a queue of more than 2^32 - 1 bytes
 * is not taken (stop = _STOP_QUEUE: the reference's uint32_t would have wrapped).
 * opts: src_host (what the same connection's sccsum_tcp_opts carries; not
 * consulted: no output holds the source address), mtu 68..65535, max_packet_len
 * 41..65535 (read only with SCCSUM_TCP_TSO), headroom 20..65535, flags:
 * SCCSUM_TCP_TSO alone.
 *
 * The rule, for an eligible connection, with used = uint32(next - una) and
 * L = TSO ? max_packet_len - 40 : min(uint16(mtu - 40), mss):
 *   T = (window == 0 || used > window) ? 0 : min(window - used, U)
 *   P = min(cwnd, L)          can_send() limits every call by cwnd, not by the
 *                             flight size: the reference's behaviour, reproduced
 *   T == 0 or P == 0: ONE segment of length 0 (get_packet calls output_one()
 *     unconditionally first: the pure ACK an output() exists to send), bytes = 0
 *   otherwise ceil(T / P) segments, segment k with seq = next + k P (mod 2^32) and
 *     len = min(P, T - k P), its bytes the stream bytes [k P, k P + len) of the
 *     concatenated buffers whatever their boundaries (whole buffers while they
 *     fit, then share(0, rest)); bytes = T
 * With P == 0 through mss == 0 (and cwnd > 0, T > 0) the reference's chain does
 * not end: can_send() stays positive and every poll sends another empty segment.
 * The call sends the one; a host should not mark such a tcb eligible.
 *
 * d_run[nconns] (32 bytes each, 16-byte aligned): segs; bytes (what the host pops
 * from its queue); seg_first, the exclusive scan of segs; next after them; flags:
 * _RTX_ARM, arm the retransmit timer now: not armed on entry and a segment with
 * len > 0 was emitted (tcp.hh:1700-1710); stop:
 *   _STOP_END         bytes == U: the queue is exhausted
 *   _STOP_WINDOW      bytes < U: the window, or segments of no bytes
 *   _STOP_INELIGIBLE  segs = 0, the state as given
 *   _STOP_QUEUE       the same, for a queue past 2^32 - 1 bytes
 *   _STOP_CAPACITY    below
 * Per segment f of the F emitted, in connection order then stream order, exactly
 * what sccsum_tcp_send takes: d_off[f] (u64) and d_len[f], the payload's place in
 * a PACKED staging layout (every segment `headroom` free bytes, then its len
 * bytes, back to back from 0); d_out[f], a complete sccsum_tcp_out {dst, seq,
 * ack = rcv_next, sport, dport, window = wnd, flags = 0x10 (f_psh and f_urg are
 * false, tcp.hh:1632-1633), hdr_len = 20 (tcp_option::get_size(false, true) is
 * 0), mss}.  d_seg_first[F + 1] and d_desc: one sccsum_gather_desc {buffer
 * address + inner offset, place in the layout, length} per (segment, buffer)
 * overlap, segment f's at [d_seg_first[f], d_seg_first[f + 1]), so
 * sccsum_gather(d_desc, d_total[2], staging) materialises every payload and the
 * same records tile the segments for sccsum_spans_desc.  Every emitted segment is
 * one unacked_segment of _snd.data; the staging copy plays the part of its clone,
 * so the application's buffers are free once the gather has run.  Pieces are at
 * most F + nbuf: d_desc has room for max_segs + nbuf records; d_off, d_len, d_out
 * for max_segs, d_seg_first for max_segs + 1.
 * d_total[4] = {segments emitted, layout bytes emitted, descriptors emitted, the
 * layout bytes needed without the caps (a connection counts as at most 2^43)}.
 * Capacity (sccsum_ipv4_send's prefix rule): connections are taken in order while
 * the segments of connections 0..c are <= max_segs (<= 2^31 - 1) and their layout
 * bytes <= max_out_bytes (<= 2^32 - 1).  From the first connection that does not
 * fit onward segs = 0, stop = _STOP_CAPACITY, seg_first = F and the state is as
 * given; no per-segment array is written past what was emitted.
 *
 * Plain dependent launches on `stream` (two tile / carry / place scans over the
 * buffers, count / scan / place over the connections, one kernel over the
 * segments), no allocation, no memset, no atomic, no payload byte moves; two
 * runs give identical bytes.  d_workspace: sccsum_tcp_tx_data_workspace(nconns,
 * nbuf) bytes, 16-byte aligned.  No output may overlap another array of the call.
 * SCCSUM_EINVAL before any device work: NULL opts or values outside the ranges
 * above, unknown flags; a NULL required pointer (d_total, d_seg_first and the
 * workspace always; with nconns != 0 d_snd, d_buf_first and d_run, the buffer
 * arrays unless nbuf == 0, the per-segment arrays unless max_segs == 0);
 * misalignment (d_snd, d_run and the workspace 16; d_buf_src, d_off, d_desc and
 * d_total 8; the 32-bit arrays and d_out 4); nconns > SCCSUM_TCP_MAX_CONNS, nbuf >
 * 2^31, max_segs > 2^31 - 1, max_out_bytes > 2^32 - 1; a stream of another device
 * than the current one.  nconns == 0 writes d_total (all 0) and d_seg_first[0]
 * and is SCCSUM_OK.  sccsum_tcp_tx_data_seg_tile() segments make one tile of the
 * segment kernel, whose grid strides past sccsum_tcp_tx_data_max_blocks(). */
#define SCCSUM_TCP_SND_ELIGIBLE  0x01u
#define SCCSUM_TCP_SND_RTX_ARMED 0x02u
#define SCCSUM_TCP_SND_RTX_ARM   0x04u /* run records only */
#define SCCSUM_TCP_STOP_QUEUE    8u

typedef struct sccsum_tcp_snd {
    uint32_t dst, next, una, window;
    uint32_t cwnd, rcv_next;
    uint16_t sport, dport, mss, wnd;
    uint8_t flags; /* SCCSUM_TCP_SND_ELIGIBLE | _RTX_ARMED */
    uint8_t pad[3];
    uint32_t reserved[3]; /* ignored */
} sccsum_tcp_snd;
typedef struct sccsum_tcp_snd_run {
    uint32_t segs, bytes, seg_first, next;
    uint8_t flags; /* SCCSUM_TCP_SND_RTX_ARM */
    uint8_t stop;  /* SCCSUM_TCP_STOP_END, _WINDOW, _INELIGIBLE, _QUEUE, _CAPACITY */
    uint16_t pad;
    uint32_t reserved[3]; /* written as 0 */
} sccsum_tcp_snd_run;
typedef struct sccsum_tcp_tx_opts {
    uint32_t src_host;       /* ipv4::_host_address, host order */
    uint32_t mtu;            /* hw_features().mtu, 68..65535 */
    uint32_t max_packet_len; /* hw_features().max_packet_len, 41..65535, with SCCSUM_TCP_TSO */
    uint32_t headroom;       /* 20..65535 */
    uint32_t flags;          /* SCCSUM_TCP_TSO */
} sccsum_tcp_tx_opts;

uint64_t sccsum_tcp_tx_data_workspace(uint32_t nconns, uint64_t nbuf);
int sccsum_tcp_tx_data_seg_tile(void);
int sccsum_tcp_tx_data_max_blocks(void);
int sccsum_tcp_tx_data(const sccsum_tcp_tx_opts* opts, const sccsum_tcp_snd* d_snd, uint32_t nconns,
                       const uint64_t* d_buf_src, const uint32_t* d_buf_len, const uint32_t* d_buf_first, uint64_t nbuf,
                       uint64_t max_segs, uint64_t max_out_bytes, sccsum_tcp_snd_run* d_run, uint64_t* d_off,
                       uint32_t* d_len, sccsum_tcp_out* d_out, uint32_t* d_seg_first, sccsum_gather_desc* d_desc,
                       uint64_t* d_total, void* d_workspace, void* stream);

/* ---- TCP ACK fast path: the advancing pure ACKs of every connection's run ---------------
 * The sender half of header prediction for a batch.  A bulk sender's inbound
 * traffic is pure ACKs that advance SND.UNA; sccsum_tcp_rx_data refuses every one
 * (_STOP_EMPTY, _STOP_ACK).  Of tcb::input_handle_other_state (include/seastar/
 * net/tcp.hh:1215-1575) such a segment takes only the advancing-ACK branch
 * (tcp.hh:1336-1400 with dupacks < 3): data_segment_acked (tcp.hh:1026-1055) with
 * update_rto (tcp.hh:2016-2039) and update_cwnd (tcp.hh:2042-2052), the window
 * update (tcp.hh:1316-1329, 1341-1343), the retransmit timer, and the closing
 * can_send() / output() (tcp.hh:1570-1574).
 *
 * sccsum_tcp_rx_acks takes the leading stretch of such ACKs of every run of
 * sccsum_tcp_rx's bucket 0 and leaves the host one record per run holding all it
 * applies to the tcb; the next sccsum_tcp_snd record follows from it without
 * touching a segment.  What is not taken, d_seg[d_run_first[r] + taken ..
 * d_run_first[r + 1]), reaches the host whole and in order, to be walked with the
 * real tcb from the state in the record: every stop is conservative and no
 * outcome depends on the device.
 *
 * Inputs: d_seg, d_first, d_run_conn, d_run_first, d_rx_total and n exactly as
 * sccsum_tcp_rx_data takes them (no host synchronisation, capturable).  No payload
 * byte is read.  d_ack[nconns] (64 bytes each, 16-byte aligned), indexed by
 * connection index, is the host's view of each tcb:
 *   una, next, window, wl1, wl2, cwnd, ssthresh, unsent_len   the _snd fields
 *                  (unacknowledged as una) as they stand
 *   rcv_next       _rcv.next
 *   rto            _rto in ms; srtt, rttvar: _snd.srtt, _snd.rttvar in ms (int64)
 *   mss            _snd.mss; window_scale: _snd.window_scale
 *   flags          SCCSUM_TCP_ACK_ELIGIBLE: set by the host only for a tcb in
 *                  ESTABLISHED or CLOSE_WAIT with _snd.dupacks < 3, _snd.window_probe
 *                  false, zero_window_probing_out == 0, _snd.window != 0 and
 *                  window_scale <= 14; _CLOSE_WAIT: the state is CLOSE_WAIT (there
 *                  tcp.hh:1522-1526 returns before the closing output());
 *                  _FIRST_SAMPLE: _snd.first_rto_sample
 *   reserved       ignored
 * The retransmit queues (_snd.data) as a CSR, as sccsum_tcp_tx_data takes its
 * buffers: connection c's entries are j in [d_q_first[c], d_q_first[c + 1])
 * (nconns + 1 entries, read as clamped into [0, nq] and non-decreasing);
 * d_q_len[j] the entry's current p.len(); d_q_meta[j] = data_len | (nr_transmits
 * != 0) << 16; d_q_tx[j] (int64) its tx_time in nanoseconds of the clock of
 * now_ns, the one clock_type::now() of the batch (lowres_clock does not move
 * inside one poll).
 *
 * The device treats a connection as _STOP_INELIGIBLE when ELIGIBLE is clear, conn
 * >= nconns, window == 0, cwnd == 0 (update_cwnd would divide by it), cwnd >=
 * 2^31, window_scale > 14 or int32(next - una) < 0; as _STOP_QUEUE when the 64-bit
 * sum of its entries' lengths is not uint32(next - una) or any entry has length
 * 0 (the reference holds none: tcp.hh:1702-1706 pushes only len > 0 and a partial
 * ACK trims strictly inside an entry).
 *
 * The rule.  Sequence numbers compare as tcp_seq does: a < b iff int32(a - b) <
 * 0 (tcp.hh:220-226).  For run r of connection c let prev be una for the run's
 * first segment and the previous segment's ack otherwise.  Segment i is taken
 * iff every earlier one was and none of these holds, tested in this order; the
 * first that holds is the run's `stop`:
 *   _STOP_INELIGIBLE, _STOP_QUEUE   above
 *   _STOP_SEQ      seq != rcv_next                      (tcp.hh:1058-1064, 1231-1245)
 *   _STOP_FLAGS    (flags & 0x37) != 0x10: FIN, SYN, RST or URG, or no ACK
 *   _STOP_DATA     pay_len != 0: text is sccsum_tcp_rx_data's business
 *   _STOP_ACK      not (prev < ack && ack <= next): a duplicate, an old ACK or one
 *                  beyond SND.NXT                       (tcp.hh:1401-1444)
 *   _STOP_WL       the run's first segment only: not (wl1 < seq || (wl1 == seq &&
 *                  wl2 <= ack)) (tcp.hh:1341; after a taken ACK wl1 == seq and wl2
 *                  == prev < ack, so it can only hold at a head)
 *   _STOP_WINDOW   (window16 << window_scale) == 0: update_window would arm the
 *                  persist timer with the _rto of that moment (tcp.hh:1323-1325)
 *   _STOP_END (0)  the run is exhausted
 * The effect of the taken ACKs is the reference's loop, literally.  For each in
 * order: pop queue entries while una + len <= ack, each pop doing una += len,
 * update_rto(tx_time) unless the entry was retransmitted, update_cwnd(len) and
 * queue_freed += data_len; then, if una < ack still, partial = ack - una trims
 * the front entry, una = ack and update_cwnd(partial); then window = window16 <<
 * window_scale.
 *   update_cwnd(bytes), uint32:  cwnd < ssthresh ? cwnd += min(bytes, mss)
 *                                                : cwnd += max(1, mss * mss / cwnd)
 *   update_rto(tx), int64 with C's truncating division:
 *     R = (now_ns - tx) / 1000000
 *     first sample: rttvar = R / 2, srtt = R, _FIRST_SAMPLE cleared; later ones:
 *     delta = |srtt - R|, rttvar = rttvar * 3 / 4 + delta / 4, srtt = srtt * 7 / 8 + R / 8
 *     rto = clamp(srtt + max(1, 4 rttvar), 1000, 60000)
 * can_send() > 0 after taken ACK i is unsent_len > 0 && uint32(next - ack_i) <
 * window_i (dupacks is 0 after exit_fast_recovery, cwnd only grows from a
 * positive value, window_i != 0).
 *
 * d_run[R] (64 bytes each, 16-byte aligned, room for min(n, nconns)): taken; una
 * after them; acked = una - una as given; popped, the entries popped; trim, the
 * bytes trimmed off the new front entry; queue_freed; window; cwnd; srtt, rttvar,
 * rto; flags: _FIRST_SAMPLE after the taken ACKs; _ALL_ACKED: the queue is empty
 * (stop the retransmit timer, signal_all_data_acked); _RTX_REARM: taken > 0 and
 * the queue is not empty (rearm at now + rto); _POLL: _CLOSE_WAIT is clear and
 * some taken ACK had can_send() > 0 (clear_delayed_ack(); output()); stop;
 * reserved words written as 0.  With taken == 0 the state fields are as given and
 * no flag but _FIRST_SAMPLE is set; a run whose conn >= nconns has them 0.
 * d_total[4] = {R, taken ACKs, popped entries, acked bytes}, 8-byte aligned.
 *
 * Plain dependent launches on `stream` (two tile / carry / place scans over the
 * queue entries, one kernel over the records, one over the runs with one lane per
 * run, one block for d_total), no allocation, no memset, no atomic; two runs give
 * identical bytes.  A run's lane walks its taken ACKs and popped entries one at
 * a time: srtt / rttvar are a truncating integer average that does not compose,
 * so one connection carrying the whole batch is the slow case.  d_workspace:
 * sccsum_tcp_rx_acks_workspace(n, nconns, nq) bytes, 16-byte aligned.  No output
 * may overlap another array of the call.  SCCSUM_EINVAL before any device work: a
 * NULL required pointer (d_total and the workspace always; d_q_first unless
 * nconns == 0; with n != 0 every other one, but d_ack only unless nconns == 0 and
 * d_q_len, d_q_meta, d_q_tx only unless nq == 0), misalignment (d_ack, d_run and
 * the workspace 16; d_seg, d_q_tx, d_total and d_rx_total 8; the 32-bit arrays
 * 4), n > 2^32 - 1, nconns > SCCSUM_TCP_MAX_CONNS, nq > 2^31, a stream of another
 * device than the current one.  n == 0 writes d_total (all 0) and is SCCSUM_OK. */
#define SCCSUM_TCP_ACK_ELIGIBLE     0x01u
#define SCCSUM_TCP_ACK_CLOSE_WAIT   0x02u
#define SCCSUM_TCP_ACK_FIRST_SAMPLE 0x04u /* sccsum_tcp_ack and run records */
#define SCCSUM_TCP_ACK_ALL_ACKED    0x08u /* run records only, as the next two */
#define SCCSUM_TCP_ACK_RTX_REARM    0x10u
#define SCCSUM_TCP_ACK_POLL         0x20u
#define SCCSUM_TCP_STOP_DATA        9u
#define SCCSUM_TCP_STOP_WL          10u

typedef struct sccsum_tcp_ack {
    uint32_t una, next, window, wl1;
    uint32_t wl2, cwnd, ssthresh, unsent_len;
    uint32_t rcv_next, rto;
    int64_t srtt, rttvar;
    uint16_t mss;
    uint8_t window_scale;
    uint8_t flags; /* SCCSUM_TCP_ACK_ELIGIBLE | _CLOSE_WAIT | _FIRST_SAMPLE */
    uint32_t reserved; /* ignored */
} sccsum_tcp_ack;
typedef struct sccsum_tcp_ack_run {
    uint32_t taken, una, acked, popped;
    uint32_t trim, queue_freed, window, cwnd;
    int64_t srtt, rttvar;
    uint32_t rto;
    uint8_t flags; /* SCCSUM_TCP_ACK_FIRST_SAMPLE | _ALL_ACKED | _RTX_REARM | _POLL */
    uint8_t stop;  /* SCCSUM_TCP_STOP_* */
    uint16_t pad;
    uint32_t reserved[2]; /* written as 0 */
} sccsum_tcp_ack_run;

uint64_t sccsum_tcp_rx_acks_workspace(uint64_t n, uint32_t nconns, uint64_t nq);
int sccsum_tcp_rx_acks(const sccsum_tcp_seg* d_seg, const uint32_t* d_first, const uint32_t* d_run_conn,
                       const uint32_t* d_run_first, const uint64_t* d_rx_total, uint64_t n, const sccsum_tcp_ack* d_ack,
                       uint32_t nconns, const uint32_t* d_q_first, const uint32_t* d_q_len, const uint32_t* d_q_meta,
                       const int64_t* d_q_tx, uint64_t nq, int64_t now_ns, sccsum_tcp_ack_run* d_run, uint64_t* d_total,
                       void* d_workspace, void* stream);

/* ---- TCP passive open: the SYNs of tcp_rx's LISTEN bucket become connections ------------
 * A segment with no tcb on a listening port takes the rest of tcp::received
 * (include/seastar/net/tcp.hh:888-929): listener->full(), the RST / ACK / SYN
 * triage, respond_with_reset, and for a SYN input_handle_listen_state
 * (tcp.hh:1115-1141): tcp_option::parse (src/net/tcp.cc:34-79), init_from_options
 * (tcp.hh:1079-1112), get_isn (tcp.hh:2067-2086) and the SYN-ACK of output_one with
 * tcp_option::fill (tcp.cc:81-138).  sccsum_tcp_listen does this for bucket 1 of a
 * finished sccsum_tcp_rx, in arrival order, up to the first segment whose outcome
 * needs a tcb made by this very batch; from there on the host walks, in order,
 * with its real _tcbs, so no outcome depends on the device.
 *
 * Inputs: the frames batch of the tcp_rx call (d_bytes, bytes_len, d_off, nbatch)
 * and its outputs d_first, d_order, d_seg, d_src as they stand on the device (no
 * host synchronisation, capturable).  The bucket is positions d_first[1] ..
 * d_first[2]; position i of the bucket (0-based, arrival order) is the rule's i.
 * m_max is the caller's upper bound of the bucket's size: it sizes the grids and
 * the workspace, and a longer bucket is read as cut to m_max.  The local address
 * of a segment is its frame's IPv4 destination, bytes 16..19 at
 * d_off[d_order[..]] (read as 0 where that lies outside the buffer); the option
 * bytes are the hdr_len - 20 bytes before pay_off (read as none where they lie
 * outside the buffer).  No payload byte is read.  d_space[65536] (device memory):
 * entry p is max_size - (_pending + _q.size()) of port p's listener at the start
 * of the batch, 0 when the port is full already.  opts, by value: isn_key, the 64
 * bytes of isn_secret::key as sixteen native words; isn_m, microseconds since the
 * epoch / 4, truncated to 32 bits; mtu (68..65535): local_mss = mtu - 40; flags:
 * SCCSUM_TCP_CSUM_OFFLOAD for the resets, as in sccsum_tcp_rx.
 *
 * The rule, p = the segment's dport:
 *   eligible       SYN set, RST and ACK clear (tcp.hh:902-914); FIN, PSH, URG and a
 *                  payload do not matter
 *   candidate      a connid's first eligible segment; its rank is the number of
 *                  earlier candidates on the same port
 *   created        a candidate with rank < d_space[p] at a position before `taken`.
 *                  _pending + _q.size() never decreases inside a batch (its only
 *                  decrement, add_connected_tcb, pushes to _q in the same step,
 *                  tcp.hh:767-772), so port p is full behind its d_space[p]-th
 *                  created candidate and stays full; with d_space[p] == 0 it is
 *                  full from the start
 *   taken          the first position whose connid has a created candidate before
 *                  it (the bucket's size when there is none): there the host's
 *                  _tcbs decides — an RST can erase a SYN_RECEIVED tcb and the
 *                  connid be created again, which changes full() behind it
 * d_class[i] for the positions before `taken`, decided in this order:
 *   SCCSUM_TCP_LISTEN_RESET   the port is full at i, RST clear (tcp.hh:890-898)
 *   SCCSUM_TCP_LISTEN_DROP    the port is full at i, RST set (tcp.hh:983-985)
 *   SCCSUM_TCP_LISTEN_DROP    RST set (tcp.hh:902-905)
 *   SCCSUM_TCP_LISTEN_RESET   ACK set (tcp.hh:907-912)
 *   SCCSUM_TCP_LISTEN_NEW     SYN set: a created candidate (tcp.hh:914-924)
 *   SCCSUM_TCP_LISTEN_DROP    no RST, ACK or SYN (tcp.hh:925-928)
 * and SCCSUM_TCP_LISTEN_LATER for every position >= taken: nothing else is
 * written for it and it creates nothing.  The host applies the records (each
 * created tcb counts in the _pending its walk uses) and then walks the positions
 * from `taken` on in order.
 *
 * Outputs (K created connections, in arrival order):
 *   d_class[m_max]  u8, as above
 *   d_new[K]        64 bytes each, 16-byte aligned, room for m_max: the connid;
 *                   pos = i; irs = SEG.SEQ; iss; snd_mss (536 when none was parsed);
 *                   local_mss; snd_wscale; rcv_wscale (7 iff a window-scale option
 *                   was parsed, else 0); snd_window = window << snd_wscale; cwnd = 2,
 *                   3 or 4 snd_mss (tcp.hh:1102-1108); ssthresh = snd_window;
 *                   rcv_window = 29200 << rcv_wscale; wl1 = SEG.SEQ, wl2 = SEG.ACK;
 *                   flags SCCSUM_TCP_NEW_*; reserved written as 0.  snd_wscale > 14
 *                   sets _WSCALE_BIG and keeps snd_window = ssthresh = window
 *                   unshifted (the reference's uint16 << shift is undefined from
 *                   some values on); the SYN-ACK does not depend on it
 *   d_synack        32 K bytes, 4-byte aligned, room for 32 m_max: slot k holds
 *                   tcp_option::fill's bytes for SYN|ACK at [32 k + 20, 32 k +
 *                   hdr_len): MSS (local_mss) iff one was received, window scale 7
 *                   iff one was received, NOP padding and EOL; hdr_len 20, 24 or 28.
 *                   The bytes from there to 32 k + 32 are written as 0; the twenty
 *                   in front are sccsum_tcp_send's and are not touched
 *   d_sa_off[K], d_sa_len[K], d_sa_out[K]   32 k + hdr_len (u64), 0, and a complete
 *                   sccsum_tcp_out: dst the foreign address, seq = iss, ack = irs +
 *                   1, the ports swapped, window 29200, flags 0x12, hdr_len, mss =
 *                   snd_mss.  With d_synack they are sccsum_tcp_send's batch as they
 *                   stand; sccsum_spans and sccsum_ipv4_send follow with no host step
 *   d_rst, d_rst_dst   the RESET segments answered exactly as sccsum_tcp_rx's list
 *                   is written, stable in arrival order; room for 20 m_max bytes
 *                   and m_max words
 *   d_total[4]      {taken, K, resets, dropped}, 8-byte aligned
 * iss = the first four digest bytes of MD5, little-endian, + isn_m, mod 2^32; the
 * message is {local_ip, foreign_ip, (local_port << 16) + foreign_port} as three
 * native words and the 64 key bytes: 76 bytes, two blocks, computed in the lane.
 *
 * The options follow tcp_option::parse's loop literally, its fixed advances
 * included (MSS by 4, window scale by 3, SACK by 2, whatever the length byte
 * says; an unknown kind by its length byte, ending at length 0).  Two deviations:
 * where the reference would read a byte at or past opt_end (a kind other than NOP
 * / EOL in the last position; an MSS or window scale whose value bytes lie past
 * the end) its behaviour is undefined, and the device ends the parse there and
 * keeps what it parsed before; and the device never reads outside [pay_off -
 * (hdr_len - 20), pay_off).
 *
 * Each connid's first eligible segment is found with a hash table in the
 * workspace: 2^bits slots of one word, 2^bits the smallest power of two >=
 * max(16, 2 m_max), the home slot sccsum_tcp_conns_slot(connid, bits), linear
 * probing; a slot holds the smallest position of its connid, decided by an atomic
 * min on that value.  Which slot a connid takes depends on arrival, the value
 * does not, and no atomic decides where an output lands: the ranks come from a
 * stable radix sort of the candidates by port (two 8-bit digits) and the lists
 * from stable compactions, so two runs give identical bytes.  Plain dependent
 * launches on `stream`, no allocation, no memset.  d_workspace:
 * sccsum_tcp_listen_workspace(m_max) bytes, 16-byte aligned.  No output may
 * overlap another array of the call.  SCCSUM_EINVAL before any device work: a
 * NULL required pointer (d_total and the workspace always; with m_max != 0 every
 * other one, d_bytes unless bytes_len == 0 and d_off unless nbatch == 0),
 * misalignment (d_new and the workspace 16; d_off, d_seg, d_sa_off and d_total 8;
 * the 32-bit arrays, d_synack, d_sa_out and d_rst 4), m_max >
 * SCCSUM_TCP_LISTEN_MAX, nbatch > 2^32 - 1, mtu outside 68..65535, unknown flags,
 * a stream of another device than the current one.  m_max == 0 writes d_total
 * (all 0) and is SCCSUM_OK. */
#define SCCSUM_TCP_LISTEN_NEW   0u
#define SCCSUM_TCP_LISTEN_RESET 1u
#define SCCSUM_TCP_LISTEN_DROP  2u
#define SCCSUM_TCP_LISTEN_LATER 3u
#define SCCSUM_TCP_LISTEN_MAX (1u << 30)
#define SCCSUM_TCP_NEW_MSS        0x01u /* _mss_received */
#define SCCSUM_TCP_NEW_WSCALE     0x02u /* _win_scale_received */
#define SCCSUM_TCP_NEW_SACK       0x04u /* _sack_received */
#define SCCSUM_TCP_NEW_WSCALE_BIG 0x08u /* snd_wscale > 14: snd_window and ssthresh are unshifted */

typedef struct sccsum_tcp_new {
    uint32_t local_ip, foreign_ip;
    uint16_t local_port, foreign_port;
    uint32_t pos;      /* the position in the bucket */
    uint32_t irs, iss;
    uint32_t snd_window, cwnd;
    uint32_t ssthresh, rcv_window;
    uint32_t wl1, wl2;
    uint16_t snd_mss, local_mss;
    uint8_t snd_wscale, rcv_wscale;
    uint8_t flags;     /* SCCSUM_TCP_NEW_* */
    uint8_t pad;
    uint32_t reserved[2]; /* written as 0 */
} sccsum_tcp_new;
typedef struct sccsum_tcp_listen_opts {
    uint32_t isn_key[16]; /* isn_secret::key */
    uint32_t isn_m;       /* microseconds since the epoch / 4, mod 2^32 */
    uint32_t mtu;         /* hw_features().mtu, 68..65535 */
    uint32_t flags;       /* SCCSUM_TCP_CSUM_OFFLOAD */
} sccsum_tcp_listen_opts;

uint64_t sccsum_tcp_listen_workspace(uint64_t m_max);
int sccsum_tcp_listen(sccsum_tcp_listen_opts opts, const void* d_bytes, uint64_t bytes_len, const uint64_t* d_off,
                      uint64_t nbatch, const uint32_t* d_first, const uint32_t* d_order, const sccsum_tcp_seg* d_seg,
                      const uint32_t* d_src, uint64_t m_max, const uint32_t* d_space, uint8_t* d_class,
                      sccsum_tcp_new* d_new, void* d_synack, uint64_t* d_sa_off, uint32_t* d_sa_len,
                      sccsum_tcp_out* d_sa_out, void* d_rst, uint32_t* d_rst_dst, uint64_t* d_total, void* d_workspace,
                      void* stream);

/* Pinned (page-locked) host memory for packet pools. */
int sccsum_host_alloc(void** p, uint64_t bytes);
int sccsum_host_free(void* p);

#ifdef __cplusplus
}
#endif

#endif /* SCCSUM_H */
