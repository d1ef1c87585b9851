// Spans of a table of bases -> bytes: what a node of the assembly graph spells (reference src/graph.cpp:133-170 builds a
// unitig's string by concatenating substr(0, edge length) of its nodes' strings, and :2042-2116 prints those strings; here a
// node is a list of spans of reads - rala_amd/host/assembly_graph.hpp - and its bytes are written once, at the output).
//
// A span {source, first, len, rc} spells out[j] = B[first + j] (rc = 0) or comp(B[first + len - 1 - j]) (rc = 1), B the
// source's row of the table, comp Sequence::create_reverse_complement's rule: A <-> T, C <-> G in upper case, every other
// byte as it is.  The output of a call is the concatenation of its spans; out_off is the exclusive scan of their lengths.
//
// One workgroup per tile of 16 KB of OUTPUT, 64 output bytes per thread in four aligned 16-byte stores (the tile and the
// thread shape of seq_gather_kernel).  Two lanes find the tile's spans by binary search in out_off; up to 256 of them are
// staged in LDS (where they begin in the output, where their bytes begin in the table, length, strand), more - thousands of
// spans of a byte or two - are read from global memory by every thread that needs them.  A thread finds the span that holds
// its first byte by binary search and walks on from there, one output word at a time:
//   a word that lies inside one span is ONE 4-byte load from wherever the span's bytes lie - the address has any alignment,
//   the hardware takes it (the table is global memory) - forwards as it is, backwards with its bytes swapped and the
//   complement applied to the four bytes at once, by arithmetic on the word;
//   a word that a span's end cuts is put together from single bytes.
// Every loop is bounded: the searches by the 32 bits of a span index, the walk by the tile's number of spans.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace rala_hip {

namespace {

constexpr uint32_t kTile = 16384;           // output bytes per workgroup
constexpr uint32_t kBlock = 256;
constexpr uint32_t kSeg = kTile / kBlock;   // 64 bytes per thread
constexpr uint32_t kMaxStaged = 256;        // spans of a tile held in LDS
static_assert(kSeg == 64, "four 16-byte stores per thread");

// 0x80 exactly in the bytes of x that are zero
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }

// the complement of four bytes at once: 'A' ^ 'T' = 0x15, 'C' ^ 'G' = 0x04 - a byte that is one of the four letters is
// flipped to its partner, every other byte (lower case, N, anything) stays
__device__ __forceinline__ uint32_t complement4(uint32_t w) {
    const uint32_t at = (zero_bytes(w ^ 0x41414141u) | zero_bytes(w ^ 0x54545454u)) >> 7;      // 0x01 in the bytes that are A or T
    const uint32_t cg = (zero_bytes(w ^ 0x43434343u) | zero_bytes(w ^ 0x47474747u)) >> 7;
    return w ^ (at * 0x15u) ^ (cg << 2);
}

// four bytes from any address of the table
__device__ __forceinline__ uint32_t load4(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// a span as a thread walks it: the output bytes [begin, end) it spells, and where its source range begins in the table
struct Cur {
    uint64_t begin, end, src;
    uint32_t rc;
};

// the spans of a tile, staged in LDS ...
struct StagedSpans {
    const uint64_t *begin, *src;
    const uint32_t *len, *rc;
    __device__ __forceinline__ uint64_t begin_of(uint32_t i) const { return begin[i]; }
    __device__ __forceinline__ Cur at(uint32_t i) const {
        Cur c;
        c.begin = begin[i]; c.end = c.begin + len[i]; c.src = src[i]; c.rc = rc[i];
        return c;
    }
};
// ... or where the caller put them
struct GlobalSpans {
    const rala_hip_span* __restrict__ spans;
    const uint64_t* __restrict__ out_off;
    const uint64_t* __restrict__ base_off;
    uint32_t first;
    __device__ __forceinline__ uint64_t begin_of(uint32_t i) const { return out_off[first + i]; }
    __device__ __forceinline__ Cur at(uint32_t i) const {
        const rala_hip_span s = spans[first + i];
        Cur c;
        c.begin = out_off[first + i]; c.end = c.begin + s.len; c.src = base_off[s.source] + s.first; c.rc = s.rc;
        return c;
    }
};

// the 64 output bytes at P0 (those in front of T1), from the tile's n spans
template <class Spans>
__device__ __forceinline__ void spell_segment(const Spans& S, uint32_t n, const uint8_t* __restrict__ bases, uint64_t P0, uint64_t T1,
                                              uint4* __restrict__ dst) {
    // the last span that begins at or in front of P0 holds it (empty spans that begin there too lie in front of that one)
    uint32_t lo = 0, hi = n;
    for (uint32_t it = 0; it < 32 && hi - lo > 1; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (S.begin_of(mid) <= P0) lo = mid; else hi = mid;
    }
    uint32_t i = lo;
    Cur c = S.at(i);
    for (uint32_t g = 0; g < 4; ++g) {
        uint32_t w[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint64_t o = P0 + 16 * g + 4 * q;
            uint32_t v = 0;
            if (o < T1) {
                while (o >= c.end && i + 1 < n) c = S.at(++i);
                if (o >= c.begin && o + 4 <= c.end) {
                    v = c.rc ? complement4(__builtin_bswap32(load4(bases + c.src + (c.end - o - 4)))) : load4(bases + c.src + (o - c.begin));
                } else {
#pragma unroll
                    for (uint32_t b = 0; b < 4; ++b) {
                        const uint64_t ob = o + b;
                        if (ob >= T1) continue;
                        while (ob >= c.end && i + 1 < n) c = S.at(++i);
                        if (ob < c.begin || ob >= c.end) continue;              // (never: the tile's spans cover it)
                        const uint32_t x = bases[c.src + (c.rc ? c.end - 1 - ob : ob - c.begin)];
                        v |= (c.rc ? complement4(x) & 0xFFu : x) << (8 * b);
                    }
                }
            }
            w[q] = v;
        }
        dst[g] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ __launch_bounds__(kBlock) void spell_kernel(SpellArgs A) {
    __shared__ uint64_t s_begin[kMaxStaged], s_src[kMaxStaged];
    __shared__ uint32_t s_len[kMaxStaged], s_rc[kMaxStaged];
    __shared__ uint32_t k_range[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t T0 = A.lo + (uint64_t)blockIdx.x * kTile;
    const uint64_t T1 = T0 + kTile < A.hi ? T0 + kTile : A.hi;
    // the spans with bytes in [T0, T1): from the last one that begins at or in front of T0 to the first that begins at or
    // behind T1 (out_off[n_spans] is the end of the output, at or behind T1)
    if (tid < 2) {
        uint32_t lo = 0, hi = A.n_spans;
        for (uint32_t it = 0; it < 33; ++it) {
            if (tid == 0 ? hi - lo <= 1 : lo >= hi) break;
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (tid == 0) {
                if (A.out_off[mid] <= T0) lo = mid; else hi = mid;
            } else {
                if (A.out_off[mid] < T1) lo = mid + 1; else hi = mid;
            }
        }
        k_range[tid] = lo;
    }
    __syncthreads();
    const uint32_t ka = k_range[0], kb = k_range[1];
    if (ka >= kb) return;                                           // (never: T0 < T1)
    const uint32_t n = kb - ka;
    const uint64_t P0 = T0 + tid * kSeg;
    uint4* dst = (uint4*)(A.out + (P0 - A.lo));
    if (n <= kMaxStaged) {
        if (tid < n) {
            const rala_hip_span s = A.spans[ka + tid];
            s_begin[tid] = A.out_off[ka + tid];
            s_src[tid] = A.base_off[s.source] + s.first;
            s_len[tid] = s.len;
            s_rc[tid] = s.rc;
        }
        __syncthreads();
        if (P0 >= T1) return;
        const StagedSpans S = {s_begin, s_src, s_len, s_rc};
        spell_segment(S, n, A.bases, P0, T1, dst);
    } else {
        if (P0 >= T1) return;
        const GlobalSpans S = {A.spans, A.out_off, A.base_off, ka};
        spell_segment(S, n, A.bases, P0, T1, dst);
    }
}

}  // namespace

uint32_t spell_tile_bytes() { return kTile; }

void launch_spell(const SpellArgs& A, hipStream_t s) {
    if (A.hi <= A.lo || !A.n_spans) return;
    const uint32_t tiles = (uint32_t)((A.hi - A.lo + kTile - 1) / kTile);
    hipLaunchKernelGGL(spell_kernel, dim3(tiles), dim3(kBlock), 0, s, A);
}

}  // namespace rala_hip
