// steer.hip — rx steering on the GPU: hash2cpu for a whole batch plus a STABLE
// partition of the batch's packet indices by destination shard (sccsum.h,
// "Rx steering").
//
// What it restates from the reference (paths relative to the reference tree):
//   device::forward_dst   include/seastar/net/net.hh:291-300
//   device::hash2cpu      net.hh:301-305
//   device::hash2qid      net.hh:287-289, dpdk override src/net/dpdk.cc:505-508
//   qp::build_sw_reta     src/net/net.cc:214-231
//
// Three dependent launches on the caller's stream (four past 31 shards), no
// block ever waiting on another one:
//   steer_count_kernel    one block per tile of kSteerTile packets: destination
//                         of every packet (-> d_cpu), per-bucket counts of the
//                         tile -> workspace[bucket][tile]
//   bucket_pass's scan    ONE block (scan_kernel): per bucket an exclusive scan
//                         over the tiles (in place), then the bucket bases ->
//                         d_first; with more than 32 buckets scan_rows_kernel
//                         (one block per bucket) and scan_totals_kernel instead
//   steer_scatter_kernel  one block per tile: destinations recomputed, each
//                         packet's offset inside its tile (bucket_pass's
//                         TileRank), index stored at d_first[bucket] +
//                         workspace[bucket][tile] + offset
// Bucket c < ncpu is shard c, bucket ncpu holds the dropped packets.  No
// atomic decides a position: the only atomics are LDS adds into the count
// kernel's histogram, whose sums do not depend on their order, so every
// output byte is a function of the inputs alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "bucket_pass.h"
#include "host_launch.h"
#include "sccsum.h"
#include "sccsum_diag.h"
#include "wire.h"

namespace steer {

using bucket_pass::pitch_of;
using host_launch::Chain;
using host_launch::device_ok;
using host_launch::misaligned;
using host_launch::upload;
using wire::status_passes;

constexpr int kBlock = 256;              // threads per block of the count / scatter kernels
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kRounds = 8;               // packets per thread: round r of a tile is its packets [256 r, 256 r + 256)
constexpr uint32_t kSteerTile = kBlock * kRounds;
constexpr int kMaxBuckets = 256;         // ncpu <= 255 shards + the drop bucket
constexpr int kScanBlock = 1024;         // threads of the one-block scan
constexpr uint32_t kRetaSize = 128;      // std::array<uint8_t, 128> (net.hh, qp::_sw_reta)
constexpr uint32_t kMaxRedir = 512;
constexpr uint32_t kMaxQueues = 256;

// What the kernels need of a map (by value in the launch).  `reta` points at
// the first row the launch uses: rows == 0 means every packet goes to `fixed`
// (dispatch from a queue that has no _sw_reta), rows == 1 that one row decides
// (dispatch), rows == hw_queues that hash2qid picks the row (hash2cpu).  A
// queue without a _sw_reta has its row filled with its own index at create,
// which is what forward_dst returns for it.
struct Params {
    const uint8_t* reta;   // device, rows x 128
    const uint8_t* redir;  // device, redir_size entries (16-byte padded), or nullptr
    uint32_t rows;
    uint32_t hw_queues;
    uint32_t redir_size;
    uint32_t table_bits;
    uint32_t ncpu;
    uint32_t fixed;
    uint32_t need;
    uint32_t reject;
};

// Tables into LDS: lds[0 .. rows*128) the reta rows, then the redir table.
__device__ __forceinline__ void load_tables(const Params& P, uint8_t* lds) {
    const uint32_t reta_units = P.rows * (kRetaSize / 16);
    const uint32_t redir_units = P.rows > 1 ? (P.redir_size + 15) / 16 : 0;
    uint4* dst = reinterpret_cast<uint4*>(lds);
    const uint4* src = reinterpret_cast<const uint4*>(P.reta);
    for (uint32_t i = threadIdx.x; i < reta_units; i += kBlock) dst[i] = src[i];
    const uint4* rsrc = reinterpret_cast<const uint4*>(P.redir);
    for (uint32_t i = threadIdx.x; i < redir_units; i += kBlock) dst[reta_units + i] = rsrc[i];
}

// Bucket of one packet: ncpu for a dropped one.
__device__ __forceinline__ uint32_t bucket_of(const Params& P, const uint8_t* lds, uint32_t hash, uint32_t st,
                                              bool has_status) {
    if (has_status && !status_passes(st, P.need, P.reject)) return P.ncpu;
    if (P.rows == 0) return P.fixed;
    uint32_t q = 0;
    if (P.rows > 1) {
        q = P.redir_size ? lds[P.rows * kRetaSize + (hash & (P.redir_size - 1))] : hash % P.hw_queues;
    }
    return lds[q * kRetaSize + ((hash >> P.table_bits) & (kRetaSize - 1))];
}

// Loads a tile's hashes and status bytes (all loads issued before any use) and
// turns them into buckets.
__device__ __forceinline__ void tile_buckets(const Params& P, const uint8_t* lds, const uint32_t* __restrict__ d_hash,
                                             const uint8_t* __restrict__ d_status, uint64_t n, uint64_t first,
                                             uint32_t (&b)[kRounds]) {
    uint32_t h[kRounds];
    uint32_t st[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint64_t i = first + uint64_t(r) * kBlock + threadIdx.x;
        h[r] = i < n ? d_hash[i] : 0u;
        st[r] = (d_status && i < n) ? d_status[i] : 0u;
    }
#pragma unroll
    for (int r = 0; r < kRounds; ++r) b[r] = bucket_of(P, lds, h[r], st[r], d_status != nullptr);
}

extern __shared__ uint4 steer_dyn_lds[];

__global__ __launch_bounds__(kBlock) void steer_count_kernel(const uint32_t* __restrict__ d_hash,
                                                             const uint8_t* __restrict__ d_status, uint64_t n,
                                                             uint8_t* __restrict__ d_cpu, uint32_t* __restrict__ ws,
                                                             uint32_t tile_pitch, Params P) {
    __shared__ uint32_t hist[kMaxBuckets];
    uint8_t* const lds = reinterpret_cast<uint8_t*>(steer_dyn_lds);
    const uint32_t buckets = P.ncpu + 1;
    load_tables(P, lds);
    bucket_pass::hist_clear(hist);
    __syncthreads();
    const uint64_t first = uint64_t(blockIdx.x) * kSteerTile;
    uint32_t b[kRounds];
    tile_buckets(P, lds, d_hash, d_status, n, first, b);
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint64_t i = first + uint64_t(r) * kBlock + threadIdx.x;
        const bool valid = i < n;
        bucket_pass::hist_add(hist, b[r], valid);
        if (valid && d_cpu) d_cpu[i] = b[r] == P.ncpu ? uint8_t(0xFF) : static_cast<uint8_t>(b[r]);
    }
    __syncthreads();
    bucket_pass::hist_store(hist, buckets, ws, tile_pitch);
}

__global__ __launch_bounds__(kBlock) void steer_scatter_kernel(const uint32_t* __restrict__ d_hash,
                                                               const uint8_t* __restrict__ d_status, uint64_t n,
                                                               const uint32_t* __restrict__ ws, uint32_t tile_pitch,
                                                               const uint32_t* __restrict__ d_first,
                                                               uint32_t* __restrict__ d_order, Params P) {
    // base[bucket]: where the tile's packets of the bucket start in d_order
    __shared__ uint32_t base[kMaxBuckets];
    bucket_pass::TileRank<kWaves, kRounds, kMaxBuckets> rank;
    uint8_t* const lds = reinterpret_cast<uint8_t*>(steer_dyn_lds);
    const uint32_t buckets = P.ncpu + 1;
    load_tables(P, lds);
    rank.clear(buckets);
    bucket_pass::bucket_base(base, buckets, d_first, ws, tile_pitch);
    __syncthreads();
    const uint64_t first = uint64_t(blockIdx.x) * kSteerTile;
    uint32_t b[kRounds];
    tile_buckets(P, lds, d_hash, d_status, n, first, b);
#pragma unroll
    for (int r = 0; r < kRounds; ++r) rank.mark(r, b[r], first + uint64_t(r) * kBlock + threadIdx.x < n);
    __syncthreads();
    rank.scan(buckets);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint64_t i = first + uint64_t(r) * kBlock + threadIdx.x;
        if (i < n) {
            const uint64_t pos = uint64_t(base[b[r]]) + rank.offset(r, b[r]);
            if (pos < n) d_order[pos] = static_cast<uint32_t>(i);  // always true for consistent inputs
        }
    }
}

// ---------------------------------------------------------------- host side

bool power_of_two(uint32_t v) { return v != 0 && (v & (v - 1)) == 0; }

// The scalar fields of a map (no table is read).
bool map_shape_ok(const sccsum_steer_map* m) {
    return m && m->ncpu >= 1 && m->ncpu <= 255 && m->hw_queues >= 1 && m->hw_queues <= kMaxQueues &&
           m->table_bits <= 31 && (m->redir_size == 0 || (power_of_two(m->redir_size) && m->redir_size <= kMaxRedir)) &&
           (m->redir != nullptr) == (m->redir_size != 0) && m->sw_reta != nullptr;
}

bool queue_has_reta(const sccsum_steer_map* m, uint32_t q) { return !m->sw_reta_set || m->sw_reta_set[q] != 0; }

// forward_dst(src, hash), net.hh:291-300; a src past the hardware queues is a
// proxy queue, which never has a _sw_reta (net.cc:173-212).
uint32_t forward_dst(const sccsum_steer_map* m, uint32_t src, uint32_t hash) {
    if (src >= m->hw_queues || !queue_has_reta(m, src)) return src;
    return m->sw_reta[src * kRetaSize + ((hash >> m->table_bits) % kRetaSize)];
}

uint32_t hash2qid(const sccsum_steer_map* m, uint32_t hash) {
    return m->redir_size ? m->redir[hash & (m->redir_size - 1)] : hash % m->hw_queues;
}

}  // namespace steer

struct sccsum_steer {
    int device = 0;
    sccsum_steer_map map{};           // scalar fields; the table pointers are the host copies below
    std::vector<uint8_t> reta;        // [hw_queues][128], rows of queues without a _sw_reta filled with the queue
    std::vector<uint8_t> has_reta;    // [hw_queues]
    uint8_t* d_tables = nullptr;      // device: reta rows, then the redir table (16-byte padded)
    uint32_t redir_off = 0;
};

extern "C" {

int sccsum_steer_tile_packets(void) { return static_cast<int>(steer::kSteerTile); }

int sccsum_steer_build_reta(const uint32_t* cpus, const float* weights, uint32_t n, uint8_t reta[128]) {
    if (!cpus || !weights || !reta || n == 0 || n > 255) return SCCSUM_EINVAL;
    for (uint32_t i = 0; i < n; ++i) {
        // the std::map iterates in ascending cpu order; 0xFF is the drop mark
        if (cpus[i] > 254 || (i && cpus[i] <= cpus[i - 1]) || !(weights[i] >= 0.0f) || std::isinf(weights[i])) {
            return SCCSUM_EINVAL;
        }
    }
    // net.cc:214-231, the same float arithmetic: accum / total * 128 in float, - 0.5 in double
    float total_weight = 0;
    for (uint32_t i = 0; i < n; ++i) total_weight += weights[i];
    float accum = 0;
    unsigned idx = 0;
    uint8_t out[steer::kRetaSize];
    for (uint32_t i = 0; i < n; ++i) {
        accum += weights[i];
        while (idx < steer::kRetaSize && idx < (accum / total_weight * steer::kRetaSize - 0.5)) {
            out[idx++] = static_cast<uint8_t>(cpus[i]);
        }
    }
    if (idx != steer::kRetaSize) return SCCSUM_EINVAL;  // a zero total: the reference would leave entries unset
    std::memcpy(reta, out, sizeof(out));
    return SCCSUM_OK;
}

uint32_t sccsum_steer_dest(const sccsum_steer_map* map, int mode, uint32_t src_cpu, uint32_t hash) {
    if (!steer::map_shape_ok(map)) return UINT32_MAX;
    if (mode == SCCSUM_STEER_DISPATCH) return steer::forward_dst(map, src_cpu, hash);
    if (mode == SCCSUM_STEER_HASH2CPU) return steer::forward_dst(map, steer::hash2qid(map, hash), hash);
    return UINT32_MAX;
}

int sccsum_steer_create(int device, const sccsum_steer_map* map, sccsum_steer** out) {
    using namespace steer;
    if (!out) return SCCSUM_EINVAL;
    *out = nullptr;
    if (!map_shape_ok(map)) return SCCSUM_EINVAL;
    for (uint32_t i = 0; i < map->redir_size; ++i) {
        if (map->redir[i] >= map->hw_queues) return SCCSUM_EINVAL;
    }
    for (uint32_t q = 0; q < map->hw_queues; ++q) {
        if (!queue_has_reta(map, q)) {
            if (q >= map->ncpu) return SCCSUM_EINVAL;  // forward_dst would return the queue itself
            continue;
        }
        for (uint32_t i = 0; i < kRetaSize; ++i) {
            if (map->sw_reta[q * kRetaSize + i] >= map->ncpu) return SCCSUM_EINVAL;
        }
    }
    int rc = device_ok(device);
    if (rc != SCCSUM_OK) return rc;
    auto* s = new (std::nothrow) sccsum_steer;
    if (!s) return static_cast<int>(hipErrorOutOfMemory);
    s->device = device;
    s->map = *map;
    s->reta.resize(size_t(map->hw_queues) * kRetaSize);
    s->has_reta.resize(map->hw_queues);
    for (uint32_t q = 0; q < map->hw_queues; ++q) {
        s->has_reta[q] = queue_has_reta(map, q);
        if (s->has_reta[q]) {
            std::memcpy(&s->reta[size_t(q) * kRetaSize], map->sw_reta + size_t(q) * kRetaSize, kRetaSize);
        } else {
            std::memset(&s->reta[size_t(q) * kRetaSize], static_cast<int>(q), kRetaSize);
        }
    }
    s->redir_off = static_cast<uint32_t>(s->reta.size());
    std::vector<uint8_t> blob(s->redir_off + ((map->redir_size + 15u) & ~15u), 0);
    std::memcpy(blob.data(), s->reta.data(), s->reta.size());
    if (map->redir_size) std::memcpy(blob.data() + s->redir_off, map->redir, map->redir_size);
    s->map.redir = nullptr;
    s->map.sw_reta = nullptr;
    s->map.sw_reta_set = nullptr;
    void* d[1];
    rc = upload(device, {{blob.data(), blob.size()}}, d);
    if (rc != SCCSUM_OK) {
        delete s;
        return rc;
    }
    s->d_tables = static_cast<uint8_t*>(d[0]);
    *out = s;
    return SCCSUM_OK;
}

int sccsum_steer_destroy(sccsum_steer* s) {
    if (!s) return SCCSUM_OK;
    const hipError_t e = host_launch::free_all({s->d_tables});
    delete s;
    return static_cast<int>(e);
}

uint64_t sccsum_steer_workspace(const sccsum_steer* s, uint64_t n) {
    if (!s) return 0;
    const uint64_t pitch = steer::pitch_of(wire::tiles_of(n, steer::kSteerTile));
    // the per-tile counts [ncpu + 1][pitch], then the bucket totals of the many-bucket scan
    return uint64_t(s->map.ncpu + 1) * pitch * 4u + steer::kMaxBuckets * 4u;
}

int sccsum_steer_run(const sccsum_steer* s, int mode, uint32_t src_cpu, const uint32_t* d_hash,
                     const uint8_t* d_status, uint32_t need, uint32_t reject, uint64_t n, uint8_t* d_cpu,
                     uint32_t* d_order, uint32_t* d_first, void* d_workspace, void* stream) {
    using namespace steer;
    if (!s || (mode != SCCSUM_STEER_DISPATCH && mode != SCCSUM_STEER_HASH2CPU)) return SCCSUM_EINVAL;
    if (!d_status && (need != 0 || reject != 0)) return SCCSUM_EINVAL;
    if (n > 0xFFFFFFFFull) return SCCSUM_EINVAL;  // packet indices are 32-bit
    if (misaligned(d_first, 4)) return SCCSUM_EINVAL;
    Params P{};
    P.hw_queues = s->map.hw_queues;
    P.redir_size = s->map.redir_size;
    P.table_bits = s->map.table_bits;
    P.ncpu = s->map.ncpu;
    P.need = need;
    P.reject = reject;
    P.redir = s->map.redir_size ? s->d_tables + s->redir_off : nullptr;
    if (mode == SCCSUM_STEER_DISPATCH) {
        if (src_cpu < s->map.hw_queues && s->has_reta[src_cpu]) {
            P.rows = 1;
            P.reta = s->d_tables + size_t(src_cpu) * kRetaSize;
        } else {
            if (src_cpu >= s->map.ncpu) return SCCSUM_EINVAL;  // forward_dst returns src_cpu itself
            P.rows = 0;
            P.fixed = src_cpu;
            P.reta = s->d_tables;
        }
    } else {
        P.rows = s->map.hw_queues;
        P.reta = s->d_tables;
    }
    if (n == 0 && !d_first) return SCCSUM_OK;
    if (!d_first) return SCCSUM_EINVAL;
    if (n > 0 && (!d_hash || misaligned(d_hash, 4) || misaligned(d_order, 4) || !d_workspace ||
                  misaligned(d_workspace, 16))) {
        return SCCSUM_EINVAL;
    }
    // the launches run on the stream's device, where the tables must lie
    const hipStream_t st = static_cast<hipStream_t>(stream);
    int cur = 0, dev = 0;
    const hipError_t e = host_launch::stream_devices(st, &cur, &dev);
    if (e != hipSuccess) return static_cast<int>(e);
    if (dev != s->device) return SCCSUM_EINVAL;

    const uint32_t ntiles = static_cast<uint32_t>(wire::tiles_of(n, kSteerTile));
    const uint32_t pitch = pitch_of(ntiles);
    const uint32_t buckets = P.ncpu + 1;
    uint32_t* const ws = static_cast<uint32_t*>(d_workspace);
    const size_t lds = size_t(P.rows) * kRetaSize + (P.rows > 1 ? ((P.redir_size + 15u) & ~15u) : 0u);
    Chain c{st};
    if (ntiles) c.launch(steer_count_kernel, dim3(ntiles), dim3(kBlock), lds, d_hash, d_status, n, d_cpu, ws, pitch, P);
    if (c.ok()) {
        c.e = bucket_pass::scan_buckets<kScanBlock, kMaxBuckets>(st, ws, ntiles, pitch, buckets, d_first,
                                                                 ws + uint64_t(buckets) * pitch);
    }
    if (ntiles && d_order) {
        c.launch(steer_scatter_kernel, dim3(ntiles), dim3(kBlock), lds, d_hash, d_status, n, ws, pitch, d_first, d_order,
                 P);
    }
    return c.rc();
}

}  // extern "C"
