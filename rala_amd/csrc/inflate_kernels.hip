// BGZF members -> text on the device (RFC 1951 raw deflate, one wavefront per member).
//
// A BGZF file (bgzip) is a chain of gzip members of at most 64 KB of text, each an independent raw-deflate stream with its
// CRC32 and text size (ISIZE) in the trailer.  The host lists the members (ingest.hip: rala_hip_bgzf_index) and ships the
// compressed bytes; here every member becomes its text at its offset in the text buffer, where the PAF tokeniser
// (ingest_kernels.hip) finds it exactly as an uncompressed file would have put it.
//
// One wavefront per member (a workgroup of 64 lanes):
//   - the member's text is staged in LDS (at most 64 KB), so back references are LDS reads, and the write to global memory is
//     one copy in whole dwords at the end;
//   - the decoder's state (bit buffer, positions) is wave-uniform: every lane runs the same decode, the values come through
//     readfirstlane, so the control flow never diverges; literals are written by lane 0, a match is copied by the whole wave
//     (byte j of it by lane j % 64 - distance < length included, from position j % distance);
//   - the compressed bytes come into the wave as two windows of 64 dwords (one per lane) and are read out with readlane; the
//     second window is loaded while the first is decoded;
//   - decode tables (a 10-bit look-up for literal/length codes, 8 bits for distances, canonical decoding for longer codes)
//     are built by the wave in LDS, counts and ranks by ballots;
//   - the CRC32 is 64 per-lane slices, combined in GF(2) (zlib's crc32_combine).
// What zlib's inflate (the host reader: io.cpp, BgzfSource::inflate_block) accepts is accepted, and nothing else: a stream that
// ends with exactly ISIZE bytes within the member's deflate bytes (what follows its final block is not read), code-length sets
// as inflate_table takes them (over-subscribed: never; incomplete: only a single code of one bit for literals/lengths and
// distances), no distance in front of the member's start, length symbols 286/287 and distance symbols 30/31 invalid, stored
// blocks with LEN = ~NLEN, and the CRC.  Anything else sets flag 8 and writes nothing of that member.
// The contract is tested (tests/test_gpu_inflate_crafted.py, both inflaters) against the case list of tests/deflate_craft.py -
// handmade streams that zlib's compressor never writes, valid and invalid - with zlib's inflate and the host reader as the verdict.
//
// Below the BGZF kernel: a single-member gzip stream by speculative decoding over chunks of the compressed bytes (its own header
// comment), and behind it what a file of several such members adds: the member find, the members' spans, the pieces' CRC.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "inflate_device.h"
#include "kernels.h"

namespace rala_hip {

namespace {


// job: one member - its deflate bytes at comp + comp_off (deflate_len of them, then CRC32 and ISIZE), its text (isize bytes,
// 1 .. 65536) to text + text_off
__global__ __launch_bounds__(kWave) void bgzf_inflate_kernel(const uint8_t* __restrict__ comp, const BgzfJob* __restrict__ jobs,
                                                              uint8_t* __restrict__ text, uint64_t text_cap, uint32_t* flags) {
    __shared__ __align__(16) uint8_t out[kMaxText + 16];
    __shared__ Lds T;
    const BgzfJob job = jobs[blockIdx.x];
    const uint32_t lane = lane_id();
    const uint32_t isize = uni(job.isize);
    if (isize == 0 || isize > kMaxText || job.text_off + isize > text_cap) {     // (the host's index never makes one)
        if (lane == 0) atomicOr(flags, 8u);
        return;
    }
    for (uint32_t e = lane; e < 256; e += kWave) {
        uint32_t r = e;
#pragma unroll
        for (int k = 0; k < 8; ++k) r = (r & 1u) ? (r >> 1) ^ kPoly : r >> 1;
        T.crc_table[e] = r;
    }
    const uint8_t* src = comp + job.comp_off;
    Input in;
    in.abase = (const uint8_t*)((uintptr_t)src & ~(uintptr_t)3);
    in.s0 = (uint32_t)((uintptr_t)src & 3u);
    in.end = in.s0 + uni(job.deflate_len);
    in.seek(in.s0);
    uint64_t bb = 0;            // bit buffer: nb bits, the stream's next bit in bit 0
    uint32_t nb = 0;
    uint32_t ip = in.s0;        // the next byte into the buffer
    const uint64_t limit = 8ull * (in.end - in.s0);
    auto consumed = [&]() { return 8ull * (ip - in.s0) - nb; };
    auto refill = [&]() {
        if (nb <= 32) {
            bb |= (uint64_t)in.fetch32(ip) << nb;
            nb += 32;
            ip += 4;
        }
    };
    auto bits = [&](uint32_t k) {           // k <= 16 after a refill
        const uint32_t v = (uint32_t)bb & ((1u << k) - 1u);
        bb >>= k;
        nb -= k;
        return v;
    };
    uint32_t pos = 0;
    bool bad = false, last = false;
    __syncthreads();
    while (!bad && !last) {
        refill();
        last = bits(1) != 0;
        const uint32_t type = bits(2);
        if (type == 0) {                                        // stored
            const uint64_t at = (consumed() + 7) & ~7ull;       // (the rest of the byte is dropped)
            const uint32_t p = in.s0 + (uint32_t)(at >> 3);
            if ((uint64_t)p + 4 > in.end) { bad = true; break; }
            in.seek(p);
            const uint32_t ln = in.fetch32(p);
            const uint32_t len = ln & 0xFFFFu;
            if ((ln >> 16) != (~len & 0xFFFFu) || (uint64_t)p + 4 + len > in.end || pos + len > isize) { bad = true; break; }
            for (uint32_t j = lane; j < len; j += kWave) out[pos + j] = in.abase[p + 4 + j];
            pos += len;
            ip = p + 4 + len;
            bb = 0;
            nb = 0;
            in.seek(ip);
            continue;
        }
        if (type == 3) { bad = true; break; }
        if (type == 1) {                                        // fixed codes (RFC 1951 3.2.6; zlib's 32 distance codes of 5 bits)
            for (uint32_t s = lane; s < 320; s += kWave) T.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
            __syncthreads();
            build_table(T.lens, 288, false, T.cnt_ll, T.sym_ll, T.lut_ll, kLitBits);
            build_table(T.lens + 288, 32, false, T.cnt_d, T.sym_d, T.lut_d, kDistBits);
        } else {                                                // dynamic codes
            refill();
            const uint32_t nlen = bits(5) + 257, ndist = bits(5) + 1, ncode = bits(4) + 4;
            if (nlen > 286 || ndist > 30) { bad = true; break; }
            if (lane < 19) T.lens_cl[lane] = 0;
            __syncthreads();
            for (uint32_t k = 0; k < ncode; ++k) {
                refill();
                const uint32_t v = bits(3);
                if (lane == 0) T.lens_cl[kClOrder[k]] = (uint8_t)v;
            }
            __syncthreads();
            if (!build_table(T.lens_cl, 19, true, T.cnt_d, T.sym_cl, T.lut_cl, kClBits)) { bad = true; break; }
            uint32_t have = 0, prev = 0;
            while (have < nlen + ndist) {
                refill();
                const uint32_t e = uni(T.lut_cl[(uint32_t)bb & ((1u << kClBits) - 1u)]);
                if (e == 0) { bad = true; break; }
                bits(e >> 9);
                const uint32_t s = e & 511u;
                if (s < 16) {
                    if (lane == 0) T.lens[have] = (uint8_t)s;
                    prev = s;
                    ++have;
                    continue;
                }
                uint32_t len = 0, copy;
                if (s == 16) {
                    if (have == 0) { bad = true; break; }
                    len = prev;
                    copy = 3 + bits(2);
                } else if (s == 17) {
                    copy = 3 + bits(3);
                } else {
                    copy = 11 + bits(7);
                }
                if (have + copy > nlen + ndist) { bad = true; break; }
                for (uint32_t j = lane; j < copy; j += kWave) T.lens[have + j] = (uint8_t)len;
                prev = len;
                have += copy;
            }
            if (bad || consumed() > limit) { bad = true; break; }
            __syncthreads();
            if (T.lens[256] == 0) { bad = true; break; }        // (no end-of-block code)
            if (!build_table(T.lens, nlen, false, T.cnt_ll, T.sym_ll, T.lut_ll, kLitBits)) { bad = true; break; }
            // (the distance lengths follow the literal/length ones directly: copied down to a place of their own)
            const uint32_t dl = lane < ndist ? T.lens[nlen + lane] : 0u;
            __syncthreads();
            if (lane < 32) T.lens[288 + lane] = (uint8_t)dl;
            __syncthreads();
            if (!build_table(T.lens + 288, ndist, false, T.cnt_d, T.sym_d, T.lut_d, kDistBits)) { bad = true; break; }
        }
        // the block's symbols
        for (;;) {
            refill();
            uint32_t e = uni(T.lut_ll[(uint32_t)bb & ((1u << kLitBits) - 1u)]);
            if (e == 0) e = uni(decode_canonical(T.cnt_ll, T.sym_ll, (uint32_t)bb, 15));
            if (e == 0) { bad = true; break; }
            bits(e >> 9);
            const uint32_t s = e & 511u;
            if (s < 256) {
                if (pos >= isize) { bad = true; break; }
                if (lane == 0) out[pos] = (uint8_t)s;
                ++pos;
            } else if (s == 256) {
                break;
            } else if (s <= 285) {
                const uint32_t k = s - 257;
                const uint32_t length = kLenBase[k] + bits(kLenExtra[k]);
                refill();
                uint32_t d = uni(T.lut_d[(uint32_t)bb & ((1u << kDistBits) - 1u)]);
                if (d == 0) d = uni(decode_canonical(T.cnt_d, T.sym_d, (uint32_t)bb, 15));
                if (d == 0 || (d & 511u) >= 30) { bad = true; break; }
                bits(d >> 9);
                const uint32_t dk = d & 511u;
                const uint32_t dist = kDistBase[dk] + bits(kDistExtra[dk]);
                if (dist > pos || pos + length > isize) { bad = true; break; }
                if (dist >= length) {
                    for (uint32_t j = lane; j < length; j += kWave) out[pos + j] = out[pos - dist + j];
                } else {
                    for (uint32_t j = lane; j < length; j += kWave) out[pos + j] = out[pos - dist + j % dist];
                }
                pos += length;
            } else {
                bad = true;
                break;
            }
            if (consumed() > limit) { bad = true; break; }
        }
        if (consumed() > limit) bad = true;
    }
    bad = bad || pos != isize;
    if (bad) {
        if (lane == 0) atomicOr(flags, 8u);
        return;
    }
    __syncthreads();
    // CRC32: lane k takes bytes [k * L, (k + 1) * L) (L dwords an odd number: the lanes' reads fall on different banks), then
    // every slice's CRC is shifted over the bytes behind it, and the wave's are summed (zlib crc32_combine)
    uint32_t L = (isize + 4 * kWave - 1) / (4 * kWave);
    L = (L | 1u) * 4u;
    const uint32_t b0 = min(lane * L, isize), b1 = min(b0 + L, isize);
    uint32_t r = 0;
    for (uint32_t i = b0; i < b1; ++i) r = T.crc_table[(r ^ out[i]) & 0xFFu] ^ (r >> 8);
    uint32_t part = b1 > b0 && isize > b1 ? multmodp(x2nmodp(isize - b1, 3), r) : r;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part ^= (uint32_t)__shfl_xor((int)part, off, kWave);
    const uint32_t crc = ~(part ^ multmodp(x2nmodp(isize, 3), 0xFFFFFFFFu));
    const uint8_t* tail = src + job.deflate_len;
    const uint32_t want = (uint32_t)tail[0] | (uint32_t)tail[1] << 8 | (uint32_t)tail[2] << 16 | (uint32_t)tail[3] << 24;
    if (uni(crc) != want) {
        if (lane == 0) atomicOr(flags, 8u);
        return;
    }
    // the text to global memory: bytes up to a dword boundary of the destination, then whole dwords, then the rest
    uint8_t* dst = text + job.text_off;
    const uint32_t head = min((uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u), isize);
    if (lane < head) dst[lane] = out[lane];
    const uint32_t n_words = (isize - head) / 4;
    const uint32_t* o32 = (const uint32_t*)out;
    const uint32_t sh = head * 8u;
    for (uint32_t k = lane; k < n_words; k += kWave) {
        const uint32_t o = head + 4 * k;
        const uint32_t a = o32[o >> 2], b = o32[(o >> 2) + 1];
        ((uint32_t*)(dst + head))[k] = sh ? (a >> sh) | (b << (32u - sh)) : a;
    }
    for (uint32_t i = head + 4 * n_words + lane; i < isize; i += kWave) dst[i] = out[i];
}


// ====================================================================================================================
// A single-member gzip stream (what gzip, pigz, Python's gzip and `minimap2 | gzip` write) -> text, by speculative decoding
// over independent chunks of the compressed bytes (the method of pugz / rapidgzip on CPUs):
//   find     every chunk but the first looks for the first bit offset in it that can start a deflate block;
//   count    every chunk with a start is decoded from there without its output - text sizes do not depend on what the 32 KB
//            in front of a chunk hold - until it lands on a later chunk's start (or the final block ends); a start that is
//            passed without being landed on is refuted.  The host follows "ended at the start of chunk j" from chunk 0:
//            the true chunks, their text offsets, the text's size - exact, so no buffer of a guessed capacity exists
//            that could overflow (the price: the true chunks are decoded twice; the first time without ring, stores or copies);
//   write    the true chunks again, into 16-bit symbols at their text offsets: a value below 256 is a byte, 0x8000 | k is
//            "byte k of the 32 768 in front of this chunk's start" - the ring in LDS starts as those markers, so a match that
//            reaches in front of the chunk copies markers, and no symbol ever points at another symbol;
//   windows  in text order, the 32 768 symbols in front of every true chunk are turned into bytes in place (a marker of
//            chunk j points into the window in front of chunk j, which is bytes already);
//   resolve  one streaming pass: every symbol to its byte in the text buffer, the CRC32 of every 16 KB of it on the way.
// Whatever this cannot prove - CRC32, ISIZE, the final block ending exactly at the trailer - is flag 8 for the caller.
// A file of several members (cat a.gz b.gz; option gzip_members) is the same stream entered anew behind every trailer: the
// member headers are found by gzip_member_find_kernel, counted from by gzip_count_kernel beside the chunks, chained by the host
// (ingest_formats.h: gzip_chain_members), and every member is proven alone - `first` on its first chunk, its floor beside
// every later chunk's text offset (windows, resolve), its CRC32 from the segments' registers and gzip_piece_crc_kernel's.

// starts[c] = the bit (from the buffer's start) where chunk c's first candidate block begins, kNoStart: none.  Chunk c covers
// the bytes [deflate_off + c * chunk_bytes, .. + chunk_bytes) below `end` (the trailer's first byte); chunk 0 starts at
// deflate_off by definition.  The lanes test 64 bit offsets at a time on the first 17 + 3 * HCLEN bits (BFINAL 0, BTYPE 2,
// HLIT and HDIST in range, the code-length code complete); what passes is probed by the whole wave, lowest offset first.
// false_sync n (tests): every n-th chunk starts at its first bit instead.
__global__ __launch_bounds__(kWave) void gzip_find_kernel(const uint8_t* __restrict__ comp, uint64_t end, uint64_t n_words, uint64_t deflate_off,
                                                           uint64_t chunk_bytes, uint32_t false_sync, uint64_t* __restrict__ starts) {
    __shared__ Lds T;
    const uint32_t c = blockIdx.x, lane = lane_id();
    if (c == 0) {
        if (lane == 0) starts[0] = 8ull * deflate_off;
        return;
    }
    const uint64_t b0 = 8ull * (deflate_off + (uint64_t)c * chunk_bytes);
    const uint64_t b1 = min(b0 + 8ull * chunk_bytes, 8ull * end);
    if (false_sync && c % false_sync == 0) {
        if (lane == 0) starts[c] = b0;
        return;
    }
    const uint64_t* words = (const uint64_t*)comp;
    uint64_t found = kNoStart;
    for (uint64_t base = b0; base < b1 && found == kNoStart; base += kWave) {
        const uint64_t b = base + lane;
        const uint64_t v = peek64(words, n_words, b);
        bool ok = b < b1 && (v & 7u) == 4u && ((v >> 3) & 31u) <= 29u && ((v >> 8) & 31u) <= 29u;
        if (ok) {
            const uint64_t w = peek64(words, n_words, b + 62);
            const uint32_t ncode = (uint32_t)((v >> 13) & 15u) + 4;
            uint32_t kraft = 0;
#pragma unroll
            for (uint32_t k = 0; k < 19; ++k) {
                const uint32_t l = (uint32_t)((k < 15 ? v >> (17 + 3 * k) : w >> (3 * (k - 15))) & 7u);
                if (k < ncode && l) kraft += 128u >> l;
            }
            ok = kraft == 128u;
        }
        uint64_t mask = __ballot(ok);
        while (mask) {
            const uint32_t first = (uint32_t)__ffsll((unsigned long long)mask) - 1u;
            mask &= mask - 1;
            if (probe_block(T, comp, end, base + first)) {
                found = base + first;
                break;
            }
        }
    }
    if (lane == 0) starts[c] = found;
}


// Block c < n_chunks: the span from chunk c's start.  Block n_chunks + k: the span from member candidate k's first block, decoded
// as a stream's first chunk (nothing lies in front of a member; the block may be stored, fixed or dynamic, final or not); it
// lands on the chunk starts behind it as a chunk's span does.  No span ever lands on a member candidate: a member is entered
// through the trailer in front of it alone (ingest_formats.h: gzip_chain_members).
__global__ __launch_bounds__(kWave) void gzip_count_kernel(const uint8_t* __restrict__ comp, uint64_t end, const uint64_t* __restrict__ starts,
                                                            uint32_t n_chunks, GzipSpan* __restrict__ spans, const GzipMemberCand* __restrict__ cands,
                                                            uint64_t deflate_off, uint64_t chunk_bytes, GzipSpan* __restrict__ mspans) {
    __shared__ Lds T;
    const uint32_t c = blockIdx.x;
    const bool member = c >= n_chunks;
    uint64_t s = member ? cands[c - n_chunks].deflate_bit : starts[c];
    uint32_t chunk = c;
    GzipSpan o = {};
    o.status = 3;                                                   // no start: nothing decoded
    if (member) {
        // the first chunk whose start can lie behind s: the one that holds s, where its start does
        uint32_t k = (uint32_t)min((s / 8 - min(s / 8, deflate_off)) / chunk_bytes, (uint64_t)n_chunks - 1);
        const uint64_t sk = starts[k];
        if (sk == kNoStart || sk <= s) ++k;
        chunk = k - 1;
        o.status = 2;                                               // (deflate bytes that begin in the last trailer or behind it)
        if (s >= 8ull * end) s = kNoStart;
    }
    if (s != kNoStart) o = inflate_span<false>(T, nullptr, comp, end, s, member || c == 0, starts, n_chunks, chunk, kNoStart, 0, nullptr);
    if (lane_id() == 0) (member ? mspans[c - n_chunks] : spans[c]) = o;
}

__global__ __launch_bounds__(kWave) void gzip_write_kernel(const uint8_t* __restrict__ comp, uint64_t end, const GzipJob* __restrict__ jobs,
                                                            uint16_t* __restrict__ sym, uint32_t* flags) {
    __shared__ __align__(16) uint16_t ring[kRing];
    __shared__ Lds T;
    const GzipJob job = jobs[blockIdx.x];
    const GzipSpan o = inflate_span<true>(T, ring, comp, end, job.start_bit, job.first != 0, nullptr, 0, 0, job.stop_bit, job.text_n,
                                          sym + job.text_off);
    const bool ok = o.text == job.text_n && o.status == (job.stop_bit == kNoStart ? 1u : 0u);
    if (!ok && lane_id() == 0) atomicOr(flags, 8u);
}

// the true chunk that holds text position p: the last j with text_off[j] <= p (text_off[0] = 0)
__device__ __forceinline__ uint32_t owner_of(const uint64_t* text_off, uint32_t n_true, uint64_t p) {
    uint32_t lo = 0, hi = n_true;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (text_off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// symbol at p (a marker) -> the byte it stands for, read from the window in front of its chunk (bytes by now); 0x8000 set:
// it points in front of its member's text (mfloor[j]: where the member of chunk j begins), or at something that is no byte
__device__ __forceinline__ uint32_t through_window(const uint16_t* sym, const uint64_t* text_off, const uint64_t* mfloor, uint32_t n_true, uint64_t p,
                                                   uint32_t s) {
    const uint32_t j = owner_of(text_off, n_true, p);
    const uint64_t src = text_off[j] + (s & 0x7FFFu);
    return src < kRing + mfloor[j] ? 0x8000u : sym[src - kRing];
}

// The windows, one workgroup, in text order: the symbols [text_off[i] - 32 768, text_off[i]) become bytes in place - 8 symbols per
// thread and load, a vector's markers looked up side by side (their chunk: i - 1, or a few steps further back where chunks are small).
__global__ __launch_bounds__(1024) void gzip_windows_kernel(uint16_t* sym, const uint64_t* __restrict__ text_off, const uint64_t* __restrict__ mfloor,
                                                            uint32_t n_true, uint32_t* flags) {
    bool wrong = false;
    for (uint32_t i = 1; i < n_true; ++i) {
        // (nothing in front of the first chunk is a symbol of this launch: a window's carry is bytes already)
        const uint64_t hi = text_off[i], lo = max((uint64_t)(hi > kRing ? hi - kRing : 0), (uint64_t)text_off[0]);
        for (uint64_t p0 = (lo & ~7ull) + 8ull * threadIdx.x; p0 < hi; p0 += 8 * 1024) {
            const uint4 q = *(const uint4*)(sym + p0);
            uint32_t w[4] = {q.x, q.y, q.z, q.w};
            bool any = false;
#pragma unroll
            for (uint32_t e = 0; e < 8; ++e) {
                const uint64_t p = p0 + e;
                const uint32_t s = (w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
                if (p >= lo && p < hi && (s & 0x8000u)) {
                    uint32_t j = i - 1;
                    while (text_off[j] > p) --j;
                    const uint64_t src = text_off[j] + (s & 0x7FFFu);
                    const uint32_t v = src < kRing + mfloor[j] ? 0x8000u : sym[src - kRing];
                    wrong = wrong || (v & 0x8000u);
                    w[e >> 1] = (w[e >> 1] & ~(0xFFFFu << (16 * (e & 1)))) | (v & 0xFFu) << (16 * (e & 1));
                    any = true;
                }
            }
            if (any) *(uint4*)(sym + p0) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        __threadfence_block();
        __syncthreads();
    }
    if (wrong) atomicOr(flags, 8u);
}

// the share of this thread's wave in the CRC register (from zero, no final inversion) of the n <= kSeg bytes staged in `out`:
// every thread takes a slice of kSegSlice bytes and shifts its register over the bytes behind it, the wave's are summed
__device__ __forceinline__ uint32_t staged_crc_part(const uint8_t* out, uint32_t n, const uint32_t* crc_table) {
    const uint32_t s0 = min(threadIdx.x * kSegSlice, n), s1 = min(s0 + kSegSlice, n);
    uint32_t r = 0;
    for (uint32_t i = s0; i < s1; ++i) r = crc_table[(r ^ out[i]) & 0xFFu] ^ (r >> 8);
    uint32_t part = s1 > s0 && n > s1 ? multmodp(x2nmodp(n - s1, 3), r) : r;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part ^= (uint32_t)__shfl_xor((int)part, off, kWave);
    return part;
}

// kSeg bytes of text per workgroup: symbols in (8 per thread and load), markers through their chunk's window, the bytes
// staged in LDS, their CRC register (from zero, no final inversion: the host chains the segments') and out in whole 16 bytes.
__global__ __launch_bounds__(kSegThreads) void gzip_resolve_kernel(const uint16_t* __restrict__ sym, const uint64_t* __restrict__ text_off,
                                                                    const uint64_t* __restrict__ mfloor, uint32_t n_true, uint64_t text_n,
                                                                    uint8_t* __restrict__ text, uint32_t* __restrict__ seg_crc, uint32_t* flags, uint64_t front) {
    __shared__ __align__(16) uint8_t out[kSeg];
    __shared__ uint32_t crc_table[256];
    __shared__ uint32_t wave_part[kSegThreads / kWave];
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kSeg;
    const uint32_t n = (uint32_t)min((uint64_t)kSeg, text_n - base);
    {
        uint32_t r = tid;
#pragma unroll
        for (int k = 0; k < 8; ++k) r = (r & 1u) ? (r >> 1) ^ kPoly : r >> 1;
        crc_table[tid] = r;
    }
    bool wrong = false;
    for (uint32_t k = 8 * tid; k < n; k += 8 * kSegThreads) {
        const uint4 q = *(const uint4*)(sym + front + base + k);    // (the buffer is readable behind text_n)
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        uint32_t b[2] = {0, 0};
#pragma unroll
        for (uint32_t e = 0; e < 8; ++e) {
            uint32_t s = (w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
            if (k + e < n && (s & 0x8000u)) {
                s = through_window(sym, text_off, mfloor, n_true, front + base + k + e, s);
                wrong = wrong || (s & 0x8000u);
            }
            b[e >> 2] |= (s & 0xFFu) << (8 * (e & 3));
        }
        *(uint2*)(out + k) = make_uint2(b[0], b[1]);
    }
    if (wrong) atomicOr(flags, 8u);
    __syncthreads();
    const uint32_t part = staged_crc_part(out, n, crc_table);
    if ((tid & (kWave - 1)) == 0) wave_part[tid / kWave] = part;
    for (uint32_t k = 16 * tid; k < n; k += 16 * kSegThreads) {
        if (k + 16 <= n) {
            *(uint4*)(text + base + k) = *(const uint4*)(out + k);
        } else {
            for (uint32_t i = k; i < n; ++i) text[base + i] = out[i];
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
        for (uint32_t k = 0; k < kSegThreads / kWave; ++k) total ^= wave_part[k];
        seg_crc[blockIdx.x] = total;
    }
}

// out[i] = symbol n + i of (the kRing symbols at sym, then the n bytes at text)
__global__ __launch_bounds__(256) void gzip_carry_kernel(const uint16_t* __restrict__ sym, const uint8_t* __restrict__ text, uint64_t n,
                                                          uint16_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kRing) return;
    const uint64_t p = n + i;
    out[i] = p < kRing ? sym[p] : (uint16_t)text[p - kRing];
}

// ---- a PIECE of a stream (a rank of a sharded run: option gzip_in_pieces) -------------------------------------------------------
// The piece's symbols lie behind a ring of kRing identity markers (0x8000 | i: "byte i of the 32 768 in front of this piece"),
// as the writing pass left them: a marker of chunk j stands for symbol text_off[j] - kRing + k, which may itself be a marker of
// an earlier chunk - the windows pass has not run, and must not have (it needs the bytes in front of the piece, which are what
// this kernel helps to find).  One lane per symbol follows its marker from chunk to chunk until it meets a byte or the ring:
// every hop lands in a strictly earlier chunk or in the ring, so n_own + 1 hops are the most there can be; a lane that needs
// more (text offsets that do not ascend) sets the flag.  Nothing is written to sym.
//   lanes [0, kRing): out[i] = symbol own_n + i of (ring ++ the piece's own own_n symbols) - the piece's OUT-window, each
//     entry a byte or a marker into the ring, that is into the piece's in-window;
//   lanes [kRing, kRing + own_n): the own symbols, counted where they end in the ring (stats[0], 64 bits) - what the piece
//     takes from the pieces in front of it; stats[2] = the longest chase in hops.
constexpr uint32_t kComposeThreads = 256;
__global__ __launch_bounds__(kComposeThreads) void gzip_window_compose_kernel(const uint16_t* __restrict__ sym, const uint64_t* __restrict__ text_off,
                                                                             uint32_t n_own, uint64_t own_n, uint16_t* __restrict__ out,
                                                                             uint32_t* __restrict__ stats, uint32_t* flags) {
    const uint64_t lane = (uint64_t)blockIdx.x * kComposeThreads + threadIdx.x;
    const bool window = lane < kRing;
    const bool live = lane < kRing + own_n;
    uint64_t p = window ? own_n + lane : lane;                      // (positions count from the ring's first symbol)
    uint32_t s = live ? sym[p] : 0u, hops = 0;
    bool lost = false;
    while ((s & 0x8000u) && p >= kRing) {
        if (hops > n_own) { lost = true; break; }
        const uint32_t j = owner_of(text_off, n_own, p);
        p = text_off[j] + (s & 0x7FFFu) - kRing;                    // text_off[j] >= kRing: the ring lies in front of the first chunk
        if (p >= kRing + own_n) { lost = true; break; }             // (never forward: text offsets that are not the chain's)
        s = sym[p];
        ++hops;
    }
    if (lost) atomicOr(flags, 8u);
    if (window) out[lane] = (uint16_t)(lost ? 0x8000u : s);
    // per wave: the own symbols that ended in the ring, the longest chase
    const unsigned long long through = __ballot(live && !window && !lost && (s & 0x8000u));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) hops = max(hops, (uint32_t)__shfl_xor((int)hops, off, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (through) atomicAdd((unsigned long long*)stats, (unsigned long long)__popcll(through));
        if (hops) atomicMax(stats + 2, hops);
    }
}

// ---- the members of a gzip file (cat a.gz b.gz, pigz -i) -----------------------------------------------------------------------
constexpr uint32_t kHeadTile = 4096;        // bytes of the file per workgroup of the member find
constexpr uint32_t kHeadThreads = 256;      // 16 bytes per thread

// ingest_formats.h's gzip_head on the bytes [off, min(n, off + kGzipHeadReach)) of comp, behind the magic, CM and the reserved
// flag bits (which the caller has seen): FEXTRA by XLEN, FNAME and FCOMMENT up to their zero byte, FHCRC skipped.  false: the
// header does not end inside those bytes.
__device__ __forceinline__ bool member_head(const uint8_t* comp, uint64_t n, uint64_t off, uint64_t* deflate_off) {
    const uint64_t lim = min(n, off + kGzipHeadReach);
    if (off + 10 > lim) return false;
    const uint32_t flg = comp[off + 3];
    uint64_t o = off + 10;
    if (flg & 4u) {
        if (o + 2 > lim) return false;
        o += 2 + ((uint32_t)comp[o] | (uint32_t)comp[o + 1] << 8);
        if (o > lim) return false;
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1) {
        if (!(flg & bit)) continue;
        while (o < lim && comp[o] != 0) ++o;
        if (o >= lim) return false;
        ++o;
    }
    if (flg & 2u) o += 2;
    if (o > lim) return false;
    *deflate_off = o;
    return true;
}

// Every byte offset of the n bytes at comp (16-byte aligned, 64 zero bytes behind them) at which a member header begins: one
// lane per 16 offsets tests 1f 8b 08 and FLG & 0xE0 == 0, what passes is parsed by member_head.  kWrite false: tile_count[t] =
// the headers that begin in tile t (the host scans them); true: tile t's headers to out[tile_first[t] ..] in ascending order,
// each with the 8 bytes in front of it.  A header may end in any later tile; its first four bytes may straddle two.  A magic
// inside deflate bytes is a candidate like any other: the chain never reaches it.
template <bool kWrite>
__global__ __launch_bounds__(kHeadThreads) void gzip_member_find_kernel(const uint8_t* __restrict__ comp, uint64_t n, uint32_t* __restrict__ tile_count,
                                                                         const uint32_t* __restrict__ tile_first, GzipMemberCand* __restrict__ out) {
    __shared__ uint32_t wave_total[kHeadThreads / kWave];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint64_t b = (uint64_t)blockIdx.x * kHeadTile + 16ull * tid;
    uint32_t w[5] = {0, 0, 0, 0, 0};
    if (b < n) {                                                    // (b + 20 <= n + 64)
        const uint4 q = *(const uint4*)(comp + b);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        w[4] = *(const uint32_t*)(comp + b + 16);
    }
    uint32_t magic = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t sh = 8u * (i & 3u);
        const uint32_t v = sh ? (w[i >> 2] >> sh) | (w[(i >> 2) + 1] << (32u - sh)) : w[i >> 2];
        if ((v & 0xE0FFFFFFu) == 0x00088B1Fu && b + i < n) magic |= 1u << i;
    }
    uint32_t heads = 0;
    for (uint32_t m = magic; m;) {
        const uint32_t i = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1;
        uint64_t d;
        if (member_head(comp, n, b + i, &d)) heads |= 1u << i;
    }
    uint32_t incl = (uint32_t)__popc(heads);
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, d, kWave);
        if (lane >= d) incl += t;
    }
    if (lane == kWave - 1) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < kHeadThreads / kWave; ++k) {
        if (k < wave) before += wave_total[k];
        total += wave_total[k];
    }
    if (!kWrite) {
        if (tid == 0) tile_count[blockIdx.x] = total;
        return;
    }
    uint64_t at = (uint64_t)tile_first[blockIdx.x] + before + incl - (uint32_t)__popc(heads);
    for (uint32_t m = heads; m;) {
        const uint32_t i = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1;
        const uint64_t off = b + i;
        uint64_t d = 0;
        member_head(comp, n, off, &d);
        GzipMemberCand c;
        c.header_off = off;
        c.deflate_bit = 8ull * d;
        c.prev_crc = c.prev_isize = 0;
        if (off >= 8) {
            const uint8_t* t = comp + off - 8;
            c.prev_crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            c.prev_isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        }
        out[at++] = c;
    }
}

// One workgroup per piece of the text (at most kSeg bytes at text + off): its CRC register, from zero and without the final
// inversion, as gzip_resolve_kernel gives one per segment - the pieces are the segments cut where a member ends.
__global__ __launch_bounds__(kSegThreads) void gzip_piece_crc_kernel(const uint8_t* __restrict__ text, const GzipPiece* __restrict__ pieces,
                                                                      uint32_t* __restrict__ reg) {
    __shared__ __align__(16) uint8_t out[kSeg];
    __shared__ uint32_t crc_table[256];
    __shared__ uint32_t wave_part[kSegThreads / kWave];
    const uint32_t tid = threadIdx.x;
    const GzipPiece pc = pieces[blockIdx.x];
    const uint32_t n = min(pc.n, kSeg);
    {
        uint32_t r = tid;
#pragma unroll
        for (int k = 0; k < 8; ++k) r = (r & 1u) ? (r >> 1) ^ kPoly : r >> 1;
        crc_table[tid] = r;
    }
    for (uint32_t k = tid; k < n; k += kSegThreads) out[k] = text[pc.off + k];
    __syncthreads();
    const uint32_t part = staged_crc_part(out, n, crc_table);
    if ((tid & (kWave - 1)) == 0) wave_part[tid / kWave] = part;
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
        for (uint32_t k = 0; k < kSegThreads / kWave; ++k) total ^= wave_part[k];
        reg[blockIdx.x] = total;
    }
}

// ---- a PIECE of a file of SEVERAL members (options gzip_in_pieces + gzip_members; the count of its candidates: inflate_members_kernels.hip)
// gzip_window_compose_kernel where the piece's own text holds member boundaries: mfloor[j] is where the member of own chunk j
// begins, in the launch's positions (0: in front of the ring or at its first symbol).  A lane's chase stops at the floor of the
// member its FIRST symbol belongs to: a hop that lands below it is a match that reaches into the member in front - nothing,
// 0x8000 in the out-window and flag 8 (zlib refuses it; followed, it would resolve to a byte of the other member's text).
// A lane that starts in the ring has no chase and no floor: what the window in front of the piece may show of it is the
// consumer's to mask (ingest_formats.h: gzip_compose_windows_masked).  stats[3] = lanes stopped at their floor.
__global__ __launch_bounds__(kComposeThreads) void gzip_window_compose_members_kernel(const uint16_t* __restrict__ sym, const uint64_t* __restrict__ text_off,
                                                                                     const uint64_t* __restrict__ mfloor, uint32_t n_own, uint64_t own_n,
                                                                                     uint16_t* __restrict__ out, uint32_t* __restrict__ stats,
                                                                                     uint32_t* flags) {
    const uint64_t lane = (uint64_t)blockIdx.x * kComposeThreads + threadIdx.x;
    const bool window = lane < kRing;
    const bool live = lane < kRing + own_n;
    uint64_t p = window ? own_n + lane : lane;                      // (positions count from the ring's first symbol)
    uint32_t s = live ? sym[p] : 0u, hops = 0;
    const uint64_t floor = live && p >= kRing ? mfloor[owner_of(text_off, n_own, p)] : 0ull;
    bool lost = false, below = false;
    while ((s & 0x8000u) && p >= kRing) {
        if (hops > n_own) { lost = true; break; }
        const uint32_t j = owner_of(text_off, n_own, p);
        p = text_off[j] + (s & 0x7FFFu) - kRing;                    // text_off[j] >= kRing: the ring lies in front of the first chunk
        if (p >= kRing + own_n) { lost = true; break; }             // (never forward: text offsets that are not the chain's)
        if (p < floor) { below = true; break; }
        s = sym[p];
        ++hops;
    }
    if (lost || below) atomicOr(flags, 8u);
    if (window) out[lane] = (uint16_t)(lost || below ? 0x8000u : s);
    // per wave: the own symbols that ended in the ring, those stopped at their floor, the longest chase
    const unsigned long long through = __ballot(live && !window && !lost && !below && (s & 0x8000u));
    const unsigned long long stopped = __ballot(below);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) hops = max(hops, (uint32_t)__shfl_xor((int)hops, off, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (through) atomicAdd((unsigned long long*)stats, (unsigned long long)__popcll(through));
        if (stopped) atomicAdd(stats + 3, (uint32_t)__popcll(stopped));
        if (hops) atomicMax(stats + 2, hops);
    }
}

constexpr X2n kX2nHost = make_x2n();
// (host) a CRC register shifted over n bytes
uint32_t crc_shift(uint32_t r, uint64_t n) {
    uint32_t p = 1u << 31, k = 3;
    while (n) {
        if (n & 1) p = multmodp(kX2nHost.v[k & 31], p);
        n >>= 1;
        ++k;
    }
    return multmodp(p, r);
}

}  // namespace

void launch_bgzf_inflate(const uint8_t* comp, const BgzfJob* jobs, uint32_t n_jobs, uint8_t* text, uint64_t text_cap, uint32_t* flags,
                         hipStream_t s) {
    if (n_jobs) hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(n_jobs), dim3(kWave), 0, s, comp, jobs, text, text_cap, flags);
}

}  // namespace rala_hip

namespace rala_hip {

uint32_t gzip_segment_bytes() { return kSeg; }

void launch_gzip_find(const uint8_t* comp, uint64_t end, uint64_t n_words, uint64_t deflate_off, uint64_t chunk_bytes, uint32_t n_chunks,
                      uint32_t false_sync, uint64_t* starts, hipStream_t s) {
    hipLaunchKernelGGL(gzip_find_kernel, dim3(n_chunks), dim3(kWave), 0, s, comp, end, n_words, deflate_off, chunk_bytes, false_sync, starts);
}

void launch_gzip_count(const uint8_t* comp, uint64_t end, const uint64_t* starts, uint32_t n_chunks, GzipSpan* spans, hipStream_t s,
                       const GzipMemberCand* cands, uint32_t n_cands, uint64_t deflate_off, uint64_t chunk_bytes, GzipSpan* mspans) {
    hipLaunchKernelGGL(gzip_count_kernel, dim3(n_chunks + n_cands), dim3(kWave), 0, s, comp, end, starts, n_chunks, spans, cands, deflate_off,
                       chunk_bytes, mspans);
}

uint32_t gzip_member_tile_bytes() { return kHeadTile; }

void launch_gzip_member_count(const uint8_t* comp, uint64_t n, uint32_t* tile_count, hipStream_t s) {
    const uint64_t n_tiles = (n + kHeadTile - 1) / kHeadTile;
    if (n_tiles) hipLaunchKernelGGL(gzip_member_find_kernel<false>, dim3((uint32_t)n_tiles), dim3(kHeadThreads), 0, s, comp, n, tile_count, nullptr, nullptr);
}

void launch_gzip_member_write(const uint8_t* comp, uint64_t n, const uint32_t* tile_first, GzipMemberCand* out, hipStream_t s) {
    const uint64_t n_tiles = (n + kHeadTile - 1) / kHeadTile;
    if (n_tiles) hipLaunchKernelGGL(gzip_member_find_kernel<true>, dim3((uint32_t)n_tiles), dim3(kHeadThreads), 0, s, comp, n, nullptr, tile_first, out);
}

void launch_gzip_piece_crc(const uint8_t* text, const GzipPiece* pieces, uint32_t n_pieces, uint32_t* reg, hipStream_t s) {
    if (n_pieces) hipLaunchKernelGGL(gzip_piece_crc_kernel, dim3(n_pieces), dim3(kSegThreads), 0, s, text, pieces, reg);
}

void launch_gzip_write(const uint8_t* comp, uint64_t end, const GzipJob* jobs, uint32_t n_jobs, uint16_t* sym, uint32_t* flags, hipStream_t s) {
    if (n_jobs) hipLaunchKernelGGL(gzip_write_kernel, dim3(n_jobs), dim3(kWave), 0, s, comp, end, jobs, sym, flags);
}

void launch_gzip_resolve(uint16_t* sym, const uint64_t* text_off, const uint64_t* mfloor, uint32_t n_true, uint64_t text_n, uint8_t* text,
                         uint32_t* seg_crc, uint32_t* flags, hipStream_t s, uint64_t front) {
    if (text_n == 0) return;
    if (n_true > 1) hipLaunchKernelGGL(gzip_windows_kernel, dim3(1), dim3(1024), 0, s, sym, text_off, mfloor, n_true, flags);
    const uint64_t n_seg = (text_n + kSeg - 1) / kSeg;
    hipLaunchKernelGGL(gzip_resolve_kernel, dim3((uint32_t)n_seg), dim3(kSegThreads), 0, s, sym, text_off, mfloor, n_true, text_n, text, seg_crc, flags,
                       front);
}

uint32_t gzip_ring_symbols() { return kRing; }

void launch_gzip_carry(uint16_t* sym, const uint8_t* text, uint64_t text_n, uint16_t* tmp, hipStream_t s) {
    hipLaunchKernelGGL(gzip_carry_kernel, dim3(kRing / 256), dim3(256), 0, s, sym, text, text_n, tmp);
    (void)hipMemcpyAsync(sym, tmp, kRing * sizeof(uint16_t), hipMemcpyDeviceToDevice, s);
}

// The find and the count over the chunks [c0, c1) alone, with the kernels as they are: both give the chunk of block 0 a special
// role (the stream's first chunk), so for c0 > 0 the launch begins one chunk earlier and that block's output is no result -
// launch_gzip_find_range writes a value of no meaning to starts[c0 - 1], and launch_gzip_count_range expects the caller to have
// put kGzipNoStart there (the block then decodes nothing); spans[c].next counts from chunk c0 - 1 then (c0 = 0: from chunk 0).
void launch_gzip_find_range(const uint8_t* comp, uint64_t end, uint64_t n_words, uint64_t deflate_off, uint64_t chunk_bytes, uint32_t c0, uint32_t c1,
                            uint32_t false_sync, uint64_t* starts, hipStream_t s) {
    if (c1 <= c0) return;
    const uint32_t lead = c0 ? 1 : 0;
    hipLaunchKernelGGL(gzip_find_kernel, dim3(c1 - c0 + lead), dim3(kWave), 0, s, comp, end, n_words, deflate_off + (uint64_t)(c0 - lead) * chunk_bytes,
                       chunk_bytes, false_sync, starts + (c0 - lead));
}

void launch_gzip_count_range(const uint8_t* comp, uint64_t end, const uint64_t* starts, uint32_t n_chunks, uint32_t c0, uint32_t c1, GzipSpan* spans,
                             hipStream_t s) {
    if (c1 <= c0) return;
    const uint32_t lead = c0 ? 1 : 0, base = c0 - lead;
    // (block b is chunk base + b; it lands on the starts behind it, to the file's last chunk)
    hipLaunchKernelGGL(gzip_count_kernel, dim3(c1 - base), dim3(kWave), 0, s, comp, end, starts + base, n_chunks - base, spans + base, nullptr, 0ull,
                       1ull, nullptr);
}

void launch_gzip_window_compose(const uint16_t* sym, const uint64_t* text_off, uint32_t n_own, uint64_t own_n, uint16_t* out, uint32_t* stats,
                                uint32_t* flags, hipStream_t s) {
    const uint64_t blocks = (kRing + own_n + kComposeThreads - 1) / kComposeThreads;
    hipLaunchKernelGGL(gzip_window_compose_kernel, dim3((uint32_t)blocks), dim3(kComposeThreads), 0, s, sym, text_off, n_own, own_n, out, stats, flags);
}

void launch_gzip_window_compose_members(const uint16_t* sym, const uint64_t* text_off, const uint64_t* mfloor, uint32_t n_own, uint64_t own_n,
                                        uint16_t* out, uint32_t* stats, uint32_t* flags, hipStream_t s) {
    const uint64_t blocks = (kRing + own_n + kComposeThreads - 1) / kComposeThreads;
    hipLaunchKernelGGL(gzip_window_compose_members_kernel, dim3((uint32_t)blocks), dim3(kComposeThreads), 0, s, sym, text_off, mfloor, n_own, own_n, out,
                       stats, flags);
}

uint32_t gzip_crc_register(const uint32_t* seg_crc, uint64_t text_n) {
    uint32_t acc = 0;
    for (uint64_t b = 0, k = 0; b < text_n; b += kSeg, ++k) acc = crc_shift(acc, std::min<uint64_t>(kSeg, text_n - b)) ^ seg_crc[k];
    return acc;
}

uint32_t gzip_crc_register_chain(const uint32_t* reg, const uint64_t* len, uint64_t n) {
    uint32_t acc = 0;
    for (uint64_t i = 0; i < n; ++i) acc = crc_shift(acc, len[i]) ^ reg[i];
    return acc;
}

uint32_t gzip_crc_chain(const uint32_t* reg, const uint64_t* len, uint64_t n) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) total += len[i];
    return ~(gzip_crc_register_chain(reg, len, n) ^ crc_shift(0xFFFFFFFFu, total));
}

uint32_t gzip_crc_of_segments(const uint32_t* seg_crc, uint64_t text_n) {
    uint32_t acc = 0;
    for (uint64_t b = 0, k = 0; b < text_n; b += kSeg, ++k) acc = crc_shift(acc, std::min<uint64_t>(kSeg, text_n - b)) ^ seg_crc[k];
    return ~(acc ^ crc_shift(0xFFFFFFFFu, text_n));
}

}  // namespace rala_hip
