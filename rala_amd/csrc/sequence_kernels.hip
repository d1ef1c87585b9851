// FASTA / FASTQ text -> one index record per read on the device: where its name and its bases lie in the text, and how many
// bases there are.
//
// Replaces the first walk over the read file (reference src/graph.cpp:249-264: bioparser's FASTA / FASTQ parser, one heap
// Sequence per read, of which only the name and the length are kept) - here rala::io::read_fasta / read_fastq behind one
// gzread (rala_amd/host/io.cpp), whose verdict these kernels reproduce byte for byte.
//
// The text goes through device memory in WINDOWS, as the overlap text does (ingest.hip): the n bytes whose events are this
// launch's, and behind them a halo in which a header line that starts in the window may end.  An EVENT is a record start in
// FASTA ('>' at byte 0 of the text or directly behind a newline) and a line start in FASTQ (record r is lines 4r .. 4r + 3).
// A STRIPPED byte is what Lines::next removes: every newline, and a carriage return directly in front of one.  Two passes:
//   count    per tile of 16 KB its events and its stripped bytes; exclusive scans give every tile its first event and the
//            stripped bytes in front of it
//   record   every event's text offset and the number of stripped bytes in front of it (the window's bases added: the only
//            state a window hands to the next one is these two running counts); the thread of a header walks that one line
//            for the name's end and the line's end - never a read
// Behind the last window a pass over the RECORDS takes spans and lengths from neighbouring events: bases = span - stripped
// bytes inside it.  A read may be longer than a tile, a window or 4 GB of text; only its length has to fit 32 bits.
// What the strict shapes do not cover - FASTQ that is not four lines per record, a name of more than a kilobyte, a header
// line longer than the halo - only raises a flag, and the caller takes the host reader.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_utils.h"
#include "kernels.h"

namespace rala_hip {

namespace {

constexpr uint32_t kTile = 16384;           // bytes of text per workgroup
constexpr uint32_t kBlock = 256;
constexpr uint32_t kSeg = kTile / kBlock;   // 64 bytes per thread: one 64-bit mask
constexpr uint32_t kHalo = 4096;            // a header line ends within this many bytes of its first one
constexpr uint32_t kMaxName = 1024;         // (the PAF tokeniser's rule)
static_assert(kSeg == 64, "one 64-bit mask per thread");

// the positions of byte c (c4 = c in all four bytes of a word) among the 64 bytes of 16 words
__device__ __forceinline__ uint64_t byte_mask(const uint32_t* w, uint32_t c4) {
    uint64_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t x = w[k] ^ c4;
        const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);     // 0x80 exactly in the zero bytes
        m |= (uint64_t)((((z >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * k);
    }
    return m;
}

struct SegMasks {
    uint64_t events, stripped;
};

// the events and the stripped bytes among the 64 bytes at text + j0 (j0 a multiple of 64); bytes at or beyond n are none.
// The byte behind the segment is read (a carriage return in its last byte): the buffer is readable beyond the last tile.
template <bool kFastq>
__device__ __forceinline__ SegMasks seg_masks(const uint8_t* __restrict__ text, uint64_t j0, uint64_t n, uint32_t first_is_start) {
    SegMasks m = {0, 0};
    if (j0 >= n) return m;
    uint32_t w[16];
    const uint4* p = (const uint4*)(text + j0);
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint4 v = p[k];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
    const uint64_t nl = byte_mask(w, 0x0A0A0A0Au), cr = byte_mask(w, 0x0D0D0D0Du);
    const uint64_t valid = j0 + 64 > n ? (1ull << (n - j0)) - 1ull : ~0ull;
    const uint64_t next_nl = text[j0 + 64] == '\n' ? 1ull << 63 : 0ull;
    const uint64_t prev_nl = (j0 == 0 ? first_is_start != 0 : text[j0 - 1] == '\n') ? 1ull : 0ull;
    m.stripped = (nl | (cr & ((nl >> 1) | next_nl))) & valid;
    m.events = ((nl << 1) | prev_nl) & valid;
    if (!kFastq) m.events &= byte_mask(w, 0x3E3E3E3Eu);         // '>'
    return m;
}

template <bool kFastq>
__global__ __launch_bounds__(kBlock) void seq_count_kernel(const uint8_t* __restrict__ text, uint64_t n, uint32_t first_is_start,
                                                            uint32_t* __restrict__ tile_events, uint32_t* __restrict__ tile_stripped) {
    __shared__ uint32_t tmp[kBlock / 64 + 1];
    const uint64_t j0 = (uint64_t)blockIdx.x * kTile + threadIdx.x * kSeg;
    const SegMasks m = seg_masks<kFastq>(text, j0, n, first_is_start);
    // (both counts of a tile are at most 16384: they ride in one word)
    const uint32_t total = block_reduce<(int)kBlock>(((uint32_t)__popcll(m.events) << 16) | (uint32_t)__popcll(m.stripped), OpAdd(), 0u, tmp);
    if (threadIdx.x == 0) {
        tile_events[blockIdx.x] = total >> 16;
        tile_stripped[blockIdx.x] = total & 0xFFFFu;
    }
}

template <bool kFastq>
__global__ __launch_bounds__(kBlock) void seq_record_kernel(SequenceWindow W, SequenceColumns out, uint32_t* __restrict__ flags) {
    __shared__ uint32_t tmp[kBlock / 64 + 1];
    const uint8_t* __restrict__ text = W.text;
    const uint64_t j0 = (uint64_t)blockIdx.x * kTile + threadIdx.x * kSeg;
    const SegMasks m = seg_masks<kFastq>(text, j0, W.n, W.first_is_start);
    uint32_t total;
    const uint32_t before = block_scan_excl<(int)kBlock>(((uint32_t)__popcll(m.events) << 16) | (uint32_t)__popcll(m.stripped), OpAdd(), 0u, tmp, total);
    const uint64_t event0 = W.event0 + W.tile_event0[blockIdx.x] + (before >> 16);
    const uint64_t stripped0 = W.stripped0 + W.tile_stripped0[blockIdx.x] + (before & 0xFFFFu);
    uint64_t events = m.events;
    while (events) {
        const uint32_t b = (uint32_t)__builtin_ctzll(events);
        events &= events - 1;
        const uint64_t below = (1ull << b) - 1ull;
        const uint64_t e = event0 + (uint64_t)__popcll(m.events & below);
        const uint64_t s = stripped0 + (uint64_t)__popcll(m.stripped & below);
        const uint64_t p = j0 + b;
        out.event_pos[e] = W.text_off + p;
        out.event_stripped[e] = s;
        uint64_t r = e;
        if (kFastq) {
            if ((e & 3u) == 2u && text[p] != '+') atomicOr(flags, kSeqNotFourLines);
            if ((e & 3u) != 0u) continue;
            // an empty header line is a blank line to read_fastq (what lies behind the text reads as zeros)
            if (text[p] == '\n' || (text[p] == '\r' && text[p + 1] == '\n')) atomicOr(flags, kSeqNotFourLines);
            r = e >> 2;
        }
        // the header line: the name from behind its first byte to the first blank, tab or line end; the line's end
        const uint64_t end = p + kHalo < W.n_avail ? p + kHalo : W.n_avail;
        uint64_t q = p + 1;
        while (q < end && q - p <= kMaxName + 1) {
            const uint8_t c = text[q];
            if (c == ' ' || c == '\t' || c == '\n') break;
            ++q;
        }
        uint64_t name_end = q;
        while (q < end && text[q] != '\n') ++q;
        uint64_t data_off, data_stripped;
        if (q < end) {
            const bool cr = q > p && text[q - 1] == '\r';           // (stripped with the newline)
            if (name_end == q && cr && q - 1 > p) name_end = q - 1;
            data_off = q + 1;
            data_stripped = s + 1 + (cr ? 1 : 0);
        } else if (q == W.n_avail && W.text_off + W.n_avail == W.text_n) {
            data_off = q;                                           // the last line, no newline behind it: nothing is stripped
            data_stripped = s;
        } else {
            atomicOr(flags, kSeqHeaderBeyondHalo);
            data_off = q;
            data_stripped = s;
        }
        if (name_end - (p + 1) > kMaxName) {
            atomicOr(flags, kSeqLongName);
            name_end = p + 1;
        }
        out.name_pos[r] = W.text_off + p + 1;
        out.name_len[r] = (uint32_t)(name_end - (p + 1));
        out.data_off[r] = W.text_off + data_off;
        out.data_stripped[r] = data_stripped;
    }
}

// the names of records [0, n) of a window into the arena, in record order; name_at: the exclusive scan of their lengths
__global__ __launch_bounds__(kBlock) void seq_names_kernel(const uint8_t* __restrict__ text, uint64_t text_off, const uint64_t* __restrict__ name_pos,
                                                            const uint32_t* __restrict__ name_len, const uint32_t* __restrict__ name_at, uint64_t n,
                                                            uint64_t arena_off, uint8_t* __restrict__ arena, uint64_t* __restrict__ name_off) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t at = arena_off + name_at[i];
    const uint8_t* src = text + (name_pos[i] - text_off);
    const uint32_t len = name_len[i];
    for (uint32_t k = 0; k < len; ++k) arena[at + k] = src[k];
    name_off[i] = at;
}

// spans and lengths from neighbouring events, behind the last window
template <bool kFastq>
__global__ __launch_bounds__(kBlock) void seq_finish_kernel(uint64_t n_records, uint64_t n_events, uint64_t text_n, uint64_t stripped_n,
                                                             SequenceColumns c, uint64_t* __restrict__ data_span, uint32_t* __restrict__ length,
                                                             uint32_t* __restrict__ flags) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_records) return;
    uint64_t off, span, len;
    if (kFastq) {
        const uint64_t e = 4 * r;
        off = c.event_pos[e + 1];
        span = c.event_pos[e + 2] - off;
        len = span - (c.event_stripped[e + 2] - c.event_stripped[e + 1]);
        const bool last = e + 4 >= n_events;
        const uint64_t q_end = last ? text_n : c.event_pos[e + 4], q_end_stripped = last ? stripped_n : c.event_stripped[e + 4];
        const uint64_t q_len = q_end - c.event_pos[e + 3] - (q_end_stripped - c.event_stripped[e + 3]);
        if (q_len != len) atomicOr(flags, kSeqNotFourLines);
        c.data_off[r] = off;
    } else {
        const bool last = r + 1 >= n_records;
        off = c.data_off[r];
        span = (last ? text_n : c.event_pos[r + 1]) - off;
        len = span - ((last ? stripped_n : c.event_stripped[r + 1]) - c.data_stripped[r]);
    }
    if (len >= (1ull << 32)) atomicOr(flags, kSeqTooLong);
    data_span[r] = span;
    length[r] = (uint32_t)len;
}

// ---- the second pass: the wanted reads' bases out of a window of the text ------------------------------------------------
// One workgroup per tile of 16 KB, 64 bytes per thread in 16-byte loads.  Where a byte goes is a function of what the index
// holds: its position, the stripped bytes in front of it (the tile's count behind a scan, as the record pass has them) and
// its read's data_off / data_stripped (G.w_adj) - a read that lies over many tiles or windows needs no carry.  The tile's
// wanted reads are found by binary search; their kept bytes are compacted into LDS behind a block scan, every read's share
// of the tile a RUN (first rank, first output index), and go out rank by rank: neighbouring lanes, neighbouring bytes.  A
// tile with more than kMaxRuns wanted reads (reads of a few bytes) stores straight from the registers instead.
constexpr uint32_t kMaxRuns = 256;

// bits [a, b) of a 64-bit mask, 0 <= a < b <= 64
__device__ __forceinline__ uint64_t bit_range(uint32_t a, uint32_t b) {
    return (b >= 64 ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull);
}

__global__ __launch_bounds__(kBlock) void seq_gather_kernel(SequenceGather G) {
    __shared__ __align__(16) uint8_t stage[kTile];
    __shared__ uint32_t run_rank[kMaxRuns], run_out[kMaxRuns];
    __shared__ uint32_t tmp[kBlock / 64 + 1];
    __shared__ uint64_t k_range[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile;
    const uint64_t t1 = t0 + kTile < G.n ? t0 + kTile : G.n;
    const uint64_t T0 = G.text_off + t0, T1 = G.text_off + t1;
    // the wanted reads with text in this tile: [first whose end lies behind T0, first that starts at or behind T1)
    if (tid < 2) {
        uint64_t lo = G.k_lo, hi = G.k_hi;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            const bool left = tid == 0 ? G.w_end[mid] <= T0 : G.w_off[mid] < T1;
            if (left) lo = mid + 1; else hi = mid;
        }
        k_range[tid] = lo;
    }
    __syncthreads();
    const uint64_t ka = k_range[0], kb = k_range[1];
    if (ka >= kb) return;                                           // (the whole workgroup: no wanted read here)
    const bool direct = kb - ka > kMaxRuns;
    const uint64_t j0 = t0 + tid * kSeg;
    const uint64_t P0 = G.text_off + j0, P1 = P0 + kSeg;
    uint32_t w[16];
    uint64_t stripped = 0, valid = 0;
    if (j0 < t1) {
        const uint4* p = (const uint4*)(G.text + j0);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint4 v = p[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
        const uint64_t nl = byte_mask(w, 0x0A0A0A0Au), cr = byte_mask(w, 0x0D0D0D0Du);
        valid = j0 + kSeg > t1 ? (1ull << (t1 - j0)) - 1ull : ~0ull;
        const uint64_t next_nl = G.text[j0 + kSeg] == '\n' ? 1ull << 63 : 0ull;
        stripped = (nl | (cr & ((nl >> 1) | next_nl))) & valid;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) w[k] = 0;
    }
    // the thread's first read, and the bytes of its 64 that lie in a wanted read
    uint64_t k0 = kb;
    if (j0 < t1) {
        uint64_t lo = ka, hi = kb;
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if (G.w_end[mid] <= P0) lo = mid + 1; else hi = mid;
        }
        k0 = lo;
    }
    uint64_t sel = 0;
    for (uint64_t k = k0; k < kb; ++k) {
        const uint64_t off = G.w_off[k], end = G.w_end[k];
        if (off >= P1) break;
        sel |= bit_range((uint32_t)((off > P0 ? off : P0) - P0), (uint32_t)((end < P1 ? end : P1) - P0));
        if (end >= P1) break;
    }
    sel &= valid & ~stripped;
    // (both counts of a tile are at most 16384: they ride in one word)
    uint32_t total;
    const uint32_t before = block_scan_excl<(int)kBlock>(((uint32_t)__popcll(stripped) << 16) | (uint32_t)__popcll(sel), OpAdd(), 0u, tmp, total);
    const uint64_t s0 = G.stripped0 + G.tile_stripped0[blockIdx.x] + (before >> 16);
    const uint32_t rank0 = before & 0xFFFFu, n_sel = total & 0xFFFFu;
    bool outside = false;
    for (uint64_t k = k0; k < kb; ++k) {
        const uint64_t off = G.w_off[k], end = G.w_end[k];
        if (off >= P1) break;
        const uint64_t adj = G.w_adj[k] - G.out_lo;
        if (direct) {
            const uint64_t mine = sel & bit_range((uint32_t)((off > P0 ? off : P0) - P0), (uint32_t)((end < P1 ? end : P1) - P0));
#pragma unroll
            for (uint32_t b = 0; b < 64; ++b) {
                if ((mine >> b) & 1ull) {
                    const uint64_t o = P0 + b - (s0 + (uint64_t)__popcll(stripped & ((1ull << b) - 1ull))) + adj;
                    if (o < G.out_n) G.out[o] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
                    else outside = true;
                }
            }
        } else if (off >= P0 || tid == 0) {
            // the read's first byte in this tile is among this thread's: its run
            const uint32_t a = (uint32_t)((off > P0 ? off : P0) - P0);
            const uint64_t below = (1ull << a) - 1ull;
            const uint64_t o = P0 + a - (s0 + (uint64_t)__popcll(stripped & below)) + adj;
            run_rank[k - ka] = rank0 + (uint32_t)__popcll(sel & below);
            run_out[k - ka] = o < G.out_n ? (uint32_t)o : 0xFFFFFFFFu;
        }
        if (end >= P1) break;
    }
    if (!direct) {
        uint32_t r = rank0;
#pragma unroll
        for (uint32_t b = 0; b < 64; ++b) {
            if ((sel >> b) & 1ull) stage[r++] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
        }
        __syncthreads();
        const uint32_t n_runs = (uint32_t)(kb - ka);
        for (uint32_t c = tid; c < n_sel; c += kBlock) {
            uint32_t lo = 0, hi = n_runs;                           // the last run that begins at or in front of rank c
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (run_rank[mid] <= c) lo = mid; else hi = mid;
            }
            const uint64_t o = (uint64_t)run_out[lo] + (c - run_rank[lo]);
            if (o < G.out_n) G.out[o] = stage[c];
            else outside = true;
        }
    }
    if (outside) atomicOr(G.flags, kSeqSliceMismatch);
}

}  // namespace

uint32_t sequence_tile_bytes() { return kTile; }

uint32_t sequence_halo_bytes() { return kHalo; }

void launch_sequence_count(const uint8_t* text, uint64_t n, bool first_is_start, bool fastq, uint32_t* tile_events, uint32_t* tile_stripped,
                           hipStream_t s) {
    const uint32_t tiles = (uint32_t)((n + kTile - 1) / kTile);
    if (!tiles) return;
    if (fastq) hipLaunchKernelGGL(seq_count_kernel<true>, dim3(tiles), dim3(kBlock), 0, s, text, n, first_is_start ? 1u : 0u, tile_events, tile_stripped);
    else hipLaunchKernelGGL(seq_count_kernel<false>, dim3(tiles), dim3(kBlock), 0, s, text, n, first_is_start ? 1u : 0u, tile_events, tile_stripped);
}

void launch_sequence_records(const SequenceWindow& W, bool fastq, const SequenceColumns& out, uint32_t* flags, hipStream_t s) {
    const uint32_t tiles = (uint32_t)((W.n + kTile - 1) / kTile);
    if (!tiles) return;
    if (fastq) hipLaunchKernelGGL(seq_record_kernel<true>, dim3(tiles), dim3(kBlock), 0, s, W, out, flags);
    else hipLaunchKernelGGL(seq_record_kernel<false>, dim3(tiles), dim3(kBlock), 0, s, W, out, flags);
}

void launch_sequence_names(const uint8_t* text, uint64_t text_off, const uint64_t* name_pos, const uint32_t* name_len, const uint32_t* name_at,
                           uint64_t n, uint64_t arena_off, uint8_t* arena, uint64_t* name_off, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(seq_names_kernel, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, text, text_off, name_pos, name_len, name_at,
                       n, arena_off, arena, name_off);
}

void launch_sequence_finish(uint64_t n_records, uint64_t n_events, uint64_t text_n, uint64_t stripped_n, bool fastq, const SequenceColumns& c,
                            uint64_t* data_span, uint32_t* length, uint32_t* flags, hipStream_t s) {
    if (!n_records) return;
    const dim3 grid((uint32_t)((n_records + kBlock - 1) / kBlock));
    if (fastq) hipLaunchKernelGGL(seq_finish_kernel<true>, grid, dim3(kBlock), 0, s, n_records, n_events, text_n, stripped_n, c, data_span, length, flags);
    else hipLaunchKernelGGL(seq_finish_kernel<false>, grid, dim3(kBlock), 0, s, n_records, n_events, text_n, stripped_n, c, data_span, length, flags);
}

void launch_sequence_gather(const SequenceGather& G, hipStream_t s) {
    const uint32_t tiles = (uint32_t)((G.n + kTile - 1) / kTile);
    if (!tiles || G.k_lo >= G.k_hi) return;
    hipLaunchKernelGGL(seq_gather_kernel, dim3(tiles), dim3(kBlock), 0, s, G);
}

}  // namespace rala_hip
