// A rank's count of the member candidates of a gzip file of SEVERAL members (options gzip_in_pieces + gzip_members): a kernel in a
// file of its own, so that the code of the kernels in inflate_kernels.hip - gzip_count_kernel, which decodes the same span - is
// what it was without it.
#include "inflate_device.h"

namespace rala_hip {

namespace {

// ---- a PIECE of a file of SEVERAL members (options gzip_in_pieces + gzip_members) -----------------------------------------------
// Block k: the span from member candidate k's first block alone - what gzip_count_kernel's blocks behind its chunks do, for a
// rank that counts the candidates whose deflate bytes begin in its own chunks and no chunk beside them.  `starts` are all chunks'.
__global__ __launch_bounds__(kWave) void gzip_count_members_kernel(const uint8_t* __restrict__ comp, uint64_t end, const uint64_t* __restrict__ starts,
                                                                    uint32_t n_chunks, const GzipMemberCand* __restrict__ cands, uint64_t deflate_off,
                                                                    uint64_t chunk_bytes, GzipSpan* __restrict__ mspans) {
    __shared__ Lds T;
    uint64_t s = cands[blockIdx.x].deflate_bit;
    // the first chunk whose start can lie behind s: the one that holds s, where its start does
    uint32_t k = (uint32_t)min((s / 8 - min(s / 8, deflate_off)) / chunk_bytes, (uint64_t)n_chunks - 1);
    const uint64_t sk = starts[k];
    if (sk == kNoStart || sk <= s) ++k;
    GzipSpan o = {};
    o.status = 2;                                                   // (deflate bytes that begin in the last trailer or behind it)
    if (s < 8ull * end) o = inflate_span<false>(T, nullptr, comp, end, s, true, starts, n_chunks, k - 1, kNoStart, 0, nullptr);
    if (lane_id() == 0) mspans[blockIdx.x] = o;
}

}  // namespace

void launch_gzip_count_members(const uint8_t* comp, uint64_t end, const uint64_t* starts, uint32_t n_chunks, const GzipMemberCand* cands,
                                uint32_t n_cands, uint64_t deflate_off, uint64_t chunk_bytes, GzipSpan* mspans, hipStream_t s) {
    if (n_cands && n_chunks) {
        hipLaunchKernelGGL(gzip_count_members_kernel, dim3(n_cands), dim3(kWave), 0, s, comp, end, starts, n_chunks, cands, deflate_off, chunk_bytes, mspans);
    }
}

}  // namespace rala_hip
