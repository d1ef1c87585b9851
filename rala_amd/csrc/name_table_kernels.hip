// The read-name table (name_table.h) built on the device, straight from the sequence index (ingest_sequences.hip: the names'
// arena, name_off, name_len in record order).
//
// Replaces the host's detour behind a device index (reference src/graph.cpp:249-264: one std::string per read into an
// unordered_map; here Graph::index_sequences' string-plus-map loop and NameTable::build, rala_amd/host/io.cpp): the same
// buckets, the same hash (name_hash_with, called with a loader over the arena), the same capacity, the same answers to every
// look-up - which key sits in which slot of a probe path is the one thing that may differ, from the host and from run to run.
// Two kernels, one behind the other on the stream:
//   insert  one lane per name, linear probing from h & mask.  A slot is claimed by ONE 64-bit compare-and-swap on the
//           bucket's first 8 bytes, {hash32, id1} together; what a lane knows about a slot is the value an agent-scope atomic
//           returned, never a plain load (the L2 is per XCD).  A taken slot is rejected on hash32; only when that matches are
//           length and bytes compared, through the OCCUPANT's entry of the index (id1 - 1 -> name_off, name_len, the arena),
//           which nobody writes during the build: no lane ever reads a half-written bucket.  A lane that meets its own name
//           raises the slot's id1 to its own where that is larger (NameTable::build: the later read takes the name), by a
//           compare-and-swap loop on the same 8 bytes.  Equal names probe the same path and slots never empty again, so they
//           always meet in one slot.
//   fill    one lane per bucket: len, off (the winning read's name_off) and head (the first min(len, 16) bytes, zero padded)
//           of every taken bucket; counts the taken buckets.
// Every probe loop ends after n_buckets steps with the error word raised: a full or damaged table makes no kernel spin.
#include <hip/hip_runtime.h>

#include "device_utils.h"
#include "kernels.h"
#include "name_table.h"

namespace rala_hip {

namespace {

constexpr uint32_t kBlock = 256;

typedef unsigned long long u64;

__device__ __forceinline__ u64 slot_load(u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// true: the slot held `expected` and holds `desired` now; false: expected = what it holds
__device__ __forceinline__ bool slot_cas(u64* p, u64& expected, u64 desired) {
    return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the m (<= 8) bytes at p, little endian, zero padded; nothing behind them is read (the arena ends with its last name)
__device__ __forceinline__ uint64_t bytes8(const uint8_t* p, uint32_t m) {
    uint64_t w = 0;
    if (m >= 8) {
        __builtin_memcpy(&w, p, 8);
    } else {
        for (uint32_t j = 0; j < m; ++j) w |= (uint64_t)p[j] << (8u * j);
    }
    return w;
}

__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t n) {
    uint32_t k = 0;
    for (; k + 8 <= n; k += 8) if (bytes8(a + k, 8) != bytes8(b + k, 8)) return false;
    return bytes8(a + k, n - k) == bytes8(b + k, n - k);
}

// stats: [0] error (a probe path of n_buckets steps), [1] the longest probe path in slots, [2] taken buckets (fill)
__global__ __launch_bounds__(kBlock) void name_insert_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ name_off,
                                                              const uint32_t* __restrict__ name_len, uint32_t n, NameBucket* bucket,
                                                              uint64_t n_buckets, uint32_t* stats) {
    __shared__ uint32_t tmp[kBlock / 64 + 1];
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t path = 0;
    if (i < n) {
        const uint8_t* name = arena + name_off[i];
        const uint32_t len = name_len[i];
        const uint64_t h = name_hash_with((uint64_t)len, [&](uint64_t k, uint64_t m) { return bytes8(name + k, (uint32_t)m); });
        const uint64_t mask = n_buckets - 1;
        const uint32_t h32 = (uint32_t)(h >> 32), id1 = (uint32_t)i + 1u;
        const u64 mine = (u64)h32 | ((u64)id1 << 32);               // {hash32, id1} as the bucket's first 8 bytes hold them
        bool done = false;
        uint64_t k = h & mask;
        for (uint64_t step = 0; step < n_buckets && !done; ++step, k = (k + 1) & mask) {
            u64* slot = (u64*)(bucket + k);
            u64 cur = slot_load(slot);
            path = (uint32_t)min(step + 1, (uint64_t)0xFFFFFFFFu);
            if ((cur >> 32) == 0) {
                cur = 0;
                if (slot_cas(slot, cur, mine)) { done = true; break; }
            }
            if ((uint32_t)cur != h32) continue;
            // equal hash32: the occupant's name through ITS entry of the index (an occupant is always some record's id)
            uint32_t occ = (uint32_t)(cur >> 32) - 1u;
            if (occ >= n) break;                                     // (a damaged slot: the error below)
            if (name_len[occ] != len || !same_bytes(arena + name_off[occ], name, len)) continue;
            // the same name again: the later read takes it
            while ((uint32_t)(cur >> 32) < id1 && !slot_cas(slot, cur, mine)) {}
            done = true;
        }
        if (!done) atomicOr(&stats[0], 1u);
    }
    const uint32_t longest = block_reduce<(int)kBlock>(path, OpMax(), 0u, tmp);
    if (threadIdx.x == 0 && longest) atomicMax(&stats[1], longest);
}

__global__ __launch_bounds__(kBlock) void name_fill_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ name_off,
                                                            const uint32_t* __restrict__ name_len, uint32_t n, NameBucket* bucket,
                                                            uint64_t n_buckets, uint32_t* stats) {
    __shared__ uint32_t tmp[kBlock / 64 + 1];
    const uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t taken = 0;
    if (k < n_buckets) {
        const uint2 key = *(const uint2*)(bucket + k);              // hash32, id1 (the insert kernel has ended)
        if (key.y != 0 && key.y - 1u < n) {
            taken = 1;
            const uint32_t len = name_len[key.y - 1u];
            const uint64_t off = name_off[key.y - 1u];
            const uint8_t* name = arena + off;
            const uint64_t h0 = bytes8(name, min(len, 8u)), h1 = len > 8 ? bytes8(name + 8, min(len - 8u, 8u)) : 0ull;
            uint4* b = (uint4*)(bucket + k);
            b[0] = make_uint4(key.x, key.y, len, (uint32_t)off);
            b[1] = make_uint4((uint32_t)h0, (uint32_t)(h0 >> 32), (uint32_t)h1, (uint32_t)(h1 >> 32));
        } else if (key.y != 0) {
            atomicOr(&stats[0], 2u);
        }
    }
    const uint32_t total = block_reduce<(int)kBlock>(taken, OpAdd(), 0u, tmp);
    if (threadIdx.x == 0 && total) atomicAdd(&stats[2], total);
}

}  // namespace

void launch_name_table_build(const uint8_t* arena, const uint64_t* name_off, const uint32_t* name_len, uint32_t n, void* buckets,
                             uint64_t n_buckets, uint32_t* stats, hipStream_t s) {
    if (n) {
        name_insert_kernel<<<dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s>>>(arena, name_off, name_len, n, (NameBucket*)buckets, n_buckets, stats);
    }
    name_fill_kernel<<<dim3((uint32_t)((n_buckets + kBlock - 1) / kBlock)), dim3(kBlock), 0, s>>>(arena, name_off, name_len, n, (NameBucket*)buckets,
                                                                                                  n_buckets, stats);
}

}  // namespace rala_hip
