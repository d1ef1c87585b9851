// Pile rows on demand (option pile_rows = 0): the coverage row of a read rebuilt from its bound events.
//
// A row is a pure function of the read's events - Pile::add_layers (reference pile.cpp:274-297) over the bounds
// pos << 1 | is_end, in uint16 arithmetic with wrap-around; after a sensitive construct the second add_layers over the
// sensitive bounds of the targets on top.  The events stay resident anyway (16 bytes per overlap), the rows (2 bytes per base)
// are what fills the device: with pile_rows = 0 nothing stores them and whoever asks for one - the getters, the digests, the
// position-space fallback of the sensitive pass - has it made here, into a scratch buffer.
//
// One workgroup of 256 threads per read, the row in tiles of kRowsTile bases.  Per tile every thread walks the read's events
// (any order, any number: nothing here has a capacity): an event in front of the tile goes into the thread's carry (begins
// minus ends), an event inside it into an LDS array of 32-bit deltas by an LDS atomic, an event behind it is passed over.  The
// carries are summed over the workgroup, the deltas scanned in stretches of 2048 positions - eight consecutive positions per
// thread, a wave scan by DPP, the wavefronts' totals through LDS - and stored as they come: 16 bytes per lane, consecutive
// lanes at consecutive addresses, 1 KiB = eight whole lines per wave instruction.  Sums are taken in 32 bits and cut to 16:
// the same value mod 2^16 as the reference's wrapping counter.
//
// kRowsTile = 8192: 32 788 B of LDS per workgroup (the deltas and the scans' five words), four workgroups (sixteen wavefronts,
// 48 VGPRs each) per compute unit - enough of them that the event loads of one hide behind the scans of the others; the cost is
// events x tiles, and a tile half the size would walk the events of a 20 kb read five times instead of three for an occupancy
// this kernel has no use for.  The deltas are 32-bit
// because the LDS has no 16-bit atomic add and two counters packed into a word would carry into each other.
//
// Nothing is shared with the run-space and position-space kernels that compute the annotations: the tests use this kernel as
// a second, independent implementation of the coverage.
#include <hip/hip_runtime.h>

#include "device_utils.h"
#include "kernels.h"

namespace rala_hip {

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kStretch = kBlock * 8;       // positions scanned and stored per step
static_assert(kRowsTile % kStretch == 0, "a tile is a whole number of stretches");

__global__ __launch_bounds__(kBlock) void pile_rows_kernel(RowsArgs A) {
    __shared__ __align__(16) int32_t delta[kRowsTile];
    __shared__ int32_t tmp[kBlock / 64 + 1];
    const uint32_t tid = threadIdx.x;
    for (uint32_t item = blockIdx.x; item < A.n_items; item += gridDim.x) {
        const uint32_t r = A.reads ? A.reads[item] : A.first + item;
        const uint32_t n = A.read_len[r];
        const uint32_t n_ev = A.ev_cnt ? (A.ev_cnt[r] < A.ev_stride ? A.ev_cnt[r] : A.ev_stride) : (A.ev_off[r + 1] - A.ev_off[r]) << A.ev_shift;
        const uint32_t* __restrict__ ev = A.ev_cnt ? A.ev + (size_t)r * A.ev_stride : A.ev + ((size_t)A.ev_off[r] << A.ev_shift);
        const uint32_t n_sens = A.sens_off ? A.sens_off[r + 1] - A.sens_off[r] : 0u;
        const uint32_t* __restrict__ sens = A.sens_off ? A.sens_ev + A.sens_off[r] : nullptr;
        uint4* __restrict__ dst = (uint4*)(A.rows + A.dst_off[r]);
        for (uint32_t t0 = 0; t0 < n; t0 += kRowsTile) {
            for (uint32_t j = tid; j < kRowsTile / 4; j += kBlock) ((int4*)delta)[j] = make_int4(0, 0, 0, 0);
            __syncthreads();
            int32_t carry = 0;
            auto take = [&](uint32_t b) {
                const uint32_t pos = b >> 1;
                const int32_t d = (b & 1u) ? -1 : 1;
                if (pos < t0) carry += d;
                else if (pos - t0 < kRowsTile) atomicAdd(&delta[pos - t0], d);
            };
            for (uint32_t k = tid; k < n_ev; k += kBlock) take(ev[k]);
            for (uint32_t k = tid; k < n_sens; k += kBlock) take(sens[k]);
            // (block_reduce's first barrier is also the one between the atomics and the scan)
            int32_t cov = block_reduce<kBlock>(carry, OpAdd(), (int32_t)0, tmp);
            for (uint32_t s0 = 0; s0 < kRowsTile && t0 + s0 < n; s0 += kStretch) {
                const int4 a = ((const int4*)delta)[(s0 >> 2) + 2 * tid], b = ((const int4*)delta)[(s0 >> 2) + 2 * tid + 1];
                const int32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                int32_t sum = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) sum += d[e];
                int32_t total;
                int32_t run = cov + block_scan_excl<kBlock>(sum, OpAdd(), (int32_t)0, tmp, total);
                const uint32_t p0 = t0 + s0 + 8 * tid;      // the thread's first position
                uint32_t v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    run += d[e];
                    v[e] = p0 + e < n ? (uint32_t)run & 0xFFFFu : 0u;      // (the padding behind the last base: zero)
                }
                if (p0 < n) dst[p0 >> 3] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
                cov += total;
            }
            __syncthreads();            // the deltas are cleared for the next tile
        }
    }
}

}  // namespace

void launch_pile_rows(const RowsArgs& args, hipStream_t stream) {
    if (args.n_items == 0) return;
    // (as many workgroups as the chip holds several times over; a workgroup loops over its share)
    const uint32_t grid = args.n_items < 16384u ? args.n_items : 16384u;
    hipLaunchKernelGGL(pile_rows_kernel, dim3(grid), dim3(kBlock), 0, stream, args);
}

}  // namespace rala_hip
