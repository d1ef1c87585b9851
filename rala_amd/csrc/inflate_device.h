// The device code the inflate kernels share (inflate_kernels.hip, inflate_members_kernels.hip): constants, the tables in LDS, the bit
// reader and one span of a deflate stream decoded by a wave.  Everything here has internal linkage: a file that includes it
// gets its own copy.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace rala_hip {

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kMaxText = 65536;
constexpr uint32_t kLitBits = 10;       // look-up bits of the literal/length table
constexpr uint32_t kDistBits = 8;       // of the distance table
constexpr uint32_t kClBits = 7;         // of the code-length code (its codes have at most 7 bits: the look-up is complete)

__constant__ uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                       4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---- CRC32 (zlib's polynomial, reflected) ----
constexpr uint32_t kPoly = 0xEDB88320u;

// a * b mod p in the reflected representation (zlib crc32.c: multmodp); a != 0
__host__ __device__ constexpr uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}
struct X2n {
    uint32_t v[32];
};
constexpr X2n make_x2n() {
    X2n t{};
    uint32_t p = 1u << 30;          // x^1
    t.v[0] = p;
    for (int n = 1; n < 32; ++n) t.v[n] = p = multmodp(p, p);
    return t;
}
__constant__ X2n kX2n = make_x2n();     // x^(2^n) mod p
// x^(n * 2^k) mod p: shifting a CRC register over n bytes is multmodp(x2nmodp(n, 3), crc)
__device__ uint32_t x2nmodp(uint32_t n, uint32_t k) {
    uint32_t p = 1u << 31;
    while (n) {
        if (n & 1) p = multmodp(kX2n.v[k & 31], p);
        n >>= 1;
        ++k;
    }
    return p;
}

struct Lds {
    uint16_t lut_ll[1u << kLitBits];      // (length << 9 | symbol), 0: longer than the look-up (or no code)
    uint16_t lut_d[1u << kDistBits];
    uint16_t lut_cl[1u << kClBits];
    uint16_t cnt_ll[16], cnt_d[16];       // codes per length (canonical decoding of the long codes)
    uint16_t sym_ll[288], sym_d[32], sym_cl[19];
    uint8_t lens[320];                    // code lengths: literal/length then distance (a dynamic header)
    uint8_t lens_cl[19];
    uint32_t crc_table[256];
};

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x; }
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t lanes_below() { return (1ull << lane_id()) - 1ull; }

// canonical decoding (puff.c's decode) of the first up to max_len bits of `bits` (first bit of the stream in bit 0) with
// per-length counts cnt[]: (length << 9 | symbol), 0 when no code of at most max_len bits matches
template <class Count>
__device__ __forceinline__ uint32_t decode_canonical(const Count& cnt, const uint16_t* sym, uint32_t bits, uint32_t max_len) {
    int code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= 15; ++len) {
        if (len > max_len) break;
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int count = (int)cnt[len];
        if (code - count < first) return (len << 9) | sym[index + (code - first)];
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return 0;
}

struct RegCounts {
    uint32_t c[16];
    __device__ __forceinline__ uint32_t operator[](uint32_t k) const { return c[k]; }
};

// the decode table of n code lengths (lens, in LDS) built by the wave; codes: the code-length code (an incomplete set is
// invalid), else literal/length or distance (incomplete only as one code of one bit).  false: zlib's inflate_table refuses the set.
__device__ bool build_table(const uint8_t* lens, uint32_t n, bool codes, uint16_t* cnt, uint16_t* sym, uint16_t* lut, uint32_t lut_bits) {
    RegCounts c;
#pragma unroll
    for (uint32_t l = 0; l < 16; ++l) c.c[l] = 0;
    for (uint32_t base = 0; base < n; base += kWave) {
        const uint32_t L = base + lane_id() < n ? lens[base + lane_id()] : 0u;
#pragma unroll
        for (uint32_t l = 1; l < 16; ++l) c.c[l] += (uint32_t)__popcll(__ballot(L == l));
    }
    int left = 1;
    uint32_t max_len = 0;
#pragma unroll
    for (uint32_t l = 1; l < 16; ++l) {
        left = (left << 1) - (int)c.c[l];
        if (c.c[l]) max_len = l;
        if (left < 0) return false;                         // over-subscribed
    }
    if (max_len != 0 && left > 0 && (codes || max_len != 1)) return false;    // incomplete
    uint32_t offs[16];
    offs[0] = offs[1] = 0;
#pragma unroll
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = offs[l] + c.c[l];
    for (uint32_t base = 0; base < n; base += kWave) {
        const uint32_t L = base + lane_id() < n ? lens[base + lane_id()] : 0u;
#pragma unroll
        for (uint32_t l = 1; l < 16; ++l) {
            const uint64_t m = __ballot(L == l);
            if (L == l) sym[offs[l] + (uint32_t)__popcll(m & lanes_below())] = (uint16_t)(base + lane_id());
            offs[l] += (uint32_t)__popcll(m);
        }
    }
    if (lane_id() == 0) {
#pragma unroll
        for (uint32_t l = 0; l < 16; ++l) cnt[l] = (uint16_t)c.c[l];
    }
    __syncthreads();
    for (uint32_t e = lane_id(); e < (1u << lut_bits); e += kWave) lut[e] = (uint16_t)decode_canonical(c, sym, e, lut_bits);
    __syncthreads();
    return true;
}

// the member's deflate bytes as the wave sees them: two windows of 64 dwords, lane i holding the dword at wb + 4i (cur) and
// wb + 256 + 4i (nxt); bytes outside [s0, end) read as zero.  Offsets are relative to the dword-aligned `abase`.
struct Input {
    const uint8_t* abase;
    uint32_t s0, end;
    uint32_t wb;
    uint32_t cur, nxt;

    __device__ __forceinline__ uint32_t load(uint32_t off) const {
        if (off >= end || off + 4 <= s0) return 0u;
        uint32_t v = *(const uint32_t*)(abase + off);
        if (off < s0) v &= 0xFFFFFFFFu << (8u * (s0 - off));
        if (off + 4 > end) v &= 0xFFFFFFFFu >> (8u * (off + 4 - end));
        return v;
    }
    __device__ __forceinline__ void seek(uint32_t ip) {
        wb = ip & ~3u;
        cur = load(wb + 4 * lane_id());
        nxt = load(wb + 256 + 4 * lane_id());
    }
    // 32 bits from byte ip on (ip >= wb, and the reads move forward by at most a window at a time)
    __device__ __forceinline__ uint32_t fetch32(uint32_t ip) {
        uint32_t w = (ip - wb) >> 2;
        if (w >= 64) {
            cur = nxt;
            wb += 256;
            w -= 64;
            nxt = load(wb + 256 + 4 * lane_id());
        }
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)w);
        const uint32_t hi = w + 1 < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)(w + 1)) : (uint32_t)__builtin_amdgcn_readlane((int)nxt, 0);
        const uint32_t sh = (ip & 3u) * 8u;
        return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
    }
};

constexpr uint64_t kNoStart = ~0ull;
constexpr uint32_t kRing = 32768;           // deflate's window: the symbols a match can reach
constexpr uint32_t kProbe = 64;             // symbols a candidate block must decode to (fewer where its end-of-block comes first)
constexpr uint32_t kFlushAt = 8192;         // unflushed symbols in the ring at which they go to global memory
constexpr uint32_t kSeg = 16384;            // bytes of text per workgroup of the resolve pass
constexpr uint32_t kSegThreads = 256;
constexpr uint32_t kSegSlice = 68;          // bytes of a thread's CRC slice (17 dwords: the threads' reads fall on different banks)

// the file's bytes as the wave sees them: Input with 64-bit offsets from the (aligned) buffer's start; bytes from `end` on read as zero
struct Stream {
    const uint8_t* base;
    uint64_t end;
    uint64_t wb;
    uint32_t cur, nxt;

    __device__ __forceinline__ uint32_t load(uint64_t off) const {
        if (off >= end) return 0u;
        uint32_t v = *(const uint32_t*)(base + off);
        if (off + 4 > end) v &= 0xFFFFFFFFu >> (8u * (uint32_t)(off + 4 - end));
        return v;
    }
    __device__ __forceinline__ void seek(uint64_t ip) {
        wb = ip & ~3ull;
        cur = load(wb + 4 * lane_id());
        nxt = load(wb + 256 + 4 * lane_id());
    }
    __device__ __forceinline__ uint32_t fetch32(uint64_t ip) {
        uint32_t w = (uint32_t)((ip - wb) >> 2);
        if (w >= 64) {
            cur = nxt;
            wb += 256;
            w -= 64;
            nxt = load(wb + 256 + 4 * lane_id());
        }
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)w);
        const uint32_t hi = w + 1 < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)(w + 1)) : (uint32_t)__builtin_amdgcn_readlane((int)nxt, 0);
        const uint32_t sh = ((uint32_t)ip & 3u) * 8u;
        return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
    }
};

// the wave's bit buffer over a Stream (wave-uniform): nb bits in bb, the stream's next bit in bit 0; ip = the next byte into it
struct Bits {
    Stream in;
    uint64_t bb;
    uint64_t ip;
    uint32_t nb;

    __device__ __forceinline__ void refill() {
        if (nb <= 32) {
            bb |= (uint64_t)in.fetch32(ip) << nb;
            nb += 32;
            ip += 4;
        }
    }
    __device__ __forceinline__ uint32_t take(uint32_t k) {          // k <= 16 after a refill
        const uint32_t v = (uint32_t)bb & ((1u << k) - 1u);
        bb >>= k;
        nb -= k;
        return v;
    }
    __device__ __forceinline__ uint64_t consumed() const { return 8ull * ip - nb; }       // bits from the buffer's start
    __device__ __forceinline__ void restart(uint64_t byte) {
        ip = byte;
        bb = 0;
        nb = 0;
        in.seek(byte);
    }
    __device__ __forceinline__ void start(const uint8_t* base, uint64_t end, uint64_t bit) {
        in.base = base;
        in.end = end;
        restart(bit >> 3);
        refill();
        take((uint32_t)bit & 7u);
    }
};

// the header of a dynamic block behind BFINAL and BTYPE (RFC 1951 3.2.7) into T's tables, as bgzf_inflate_kernel reads it;
// false: zlib's inflate refuses it
__device__ __forceinline__ bool read_dynamic(Bits& r, Lds& T, uint64_t limit) {
    const uint32_t lane = lane_id();
    r.refill();
    const uint32_t nlen = r.take(5) + 257, ndist = r.take(5) + 1, ncode = r.take(4) + 4;
    if (nlen > 286 || ndist > 30) return false;
    __syncthreads();
    if (lane < 19) T.lens_cl[lane] = 0;
    __syncthreads();
    for (uint32_t k = 0; k < ncode; ++k) {
        r.refill();
        const uint32_t v = r.take(3);
        if (lane == 0) T.lens_cl[kClOrder[k]] = (uint8_t)v;
    }
    __syncthreads();
    if (!build_table(T.lens_cl, 19, true, T.cnt_d, T.sym_cl, T.lut_cl, kClBits)) return false;
    uint32_t have = 0, prev = 0;
    while (have < nlen + ndist) {
        r.refill();
        const uint32_t e = uni(T.lut_cl[(uint32_t)r.bb & ((1u << kClBits) - 1u)]);
        if (e == 0) return false;
        r.take(e >> 9);
        const uint32_t s = e & 511u;
        if (s < 16) {
            if (lane == 0) T.lens[have] = (uint8_t)s;
            prev = s;
            ++have;
            continue;
        }
        uint32_t len = 0, copy;
        if (s == 16) {
            if (have == 0) return false;
            len = prev;
            copy = 3 + r.take(2);
        } else if (s == 17) {
            copy = 3 + r.take(3);
        } else {
            copy = 11 + r.take(7);
        }
        if (have + copy > nlen + ndist) return false;
        for (uint32_t j = lane; j < copy; j += kWave) T.lens[have + j] = (uint8_t)len;
        prev = len;
        have += copy;
        if (r.consumed() > limit) return false;
    }
    if (r.consumed() > limit) return false;
    __syncthreads();
    if (T.lens[256] == 0) return false;                     // (no end-of-block code)
    if (!build_table(T.lens, nlen, false, T.cnt_ll, T.sym_ll, T.lut_ll, kLitBits)) return false;
    const uint32_t dl = lane < ndist ? T.lens[nlen + lane] : 0u;
    __syncthreads();
    if (lane < 32) T.lens[288 + lane] = (uint8_t)dl;
    __syncthreads();
    return build_table(T.lens + 288, ndist, false, T.cnt_d, T.sym_d, T.lut_d, kDistBits);
}

__device__ __forceinline__ void build_fixed(Lds& T) {
    __syncthreads();
    for (uint32_t s = lane_id(); s < 320; s += kWave) T.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
    __syncthreads();
    build_table(T.lens, 288, false, T.cnt_ll, T.sym_ll, T.lut_ll, kLitBits);
    build_table(T.lens + 288, 32, false, T.cnt_d, T.sym_d, T.lut_d, kDistBits);
}

// 64 bits of the stream from bit `bit` on (words = the buffer's 8-byte words; behind them zero)
__device__ __forceinline__ uint64_t peek64(const uint64_t* words, uint64_t n_words, uint64_t bit) {
    const uint64_t i = bit >> 6;
    const uint32_t sh = (uint32_t)bit & 63u;
    const uint64_t a = i < n_words ? words[i] : 0ull, b = i + 1 < n_words ? words[i + 1] : 0ull;
    return sh ? (a >> sh) | (b << (64u - sh)) : a;
}

// does a deflate block that can be a chunk's start begin at `bit`?  A non-final dynamic block (wave-uniform; the lanes have
// looked at the first 74 bits already, this reads them again) whose tables zlib takes and whose first kProbe symbols are
// valid codes, the literals among them text
__device__ __forceinline__ bool probe_block(Lds& T, const uint8_t* comp, uint64_t end, uint64_t bit) {
    const uint64_t limit = 8ull * end;
    Bits r;
    r.start(comp, end, bit);
    r.refill();
    if (r.take(3) != 4u) return false;
    if (!read_dynamic(r, T, limit)) return false;
    for (uint32_t n = 0; n < kProbe; ++n) {
        r.refill();
        uint32_t e = uni(T.lut_ll[(uint32_t)r.bb & ((1u << kLitBits) - 1u)]);
        if (e == 0) e = uni(decode_canonical(T.cnt_ll, T.sym_ll, (uint32_t)r.bb, 15));
        if (e == 0) return false;
        r.take(e >> 9);
        const uint32_t s = e & 511u;
        if (s < 256) {
            if (!(s == '\t' || s == '\n' || (s >= 0x20 && s <= 0x7e))) return false;
        } else if (s == 256) {
            break;
        } else if (s <= 285) {
            const uint32_t k = s - 257;
            r.take(kLenExtra[k]);
            r.refill();
            uint32_t d = uni(T.lut_d[(uint32_t)r.bb & ((1u << kDistBits) - 1u)]);
            if (d == 0) d = uni(decode_canonical(T.cnt_d, T.sym_d, (uint32_t)r.bb, 15));
            if (d == 0 || (d & 511u) >= 30) return false;           // (a valid distance code is a distance within 32 768)
            r.take(d >> 9);
            r.take(kDistExtra[d & 511u]);
        } else {
            return false;
        }
        if (r.consumed() > limit) return false;
    }
    return r.consumed() <= limit;
}

// One span of the stream decoded by the wave from start_bit (the control flow of bgzf_inflate_kernel).  first: the stream's
// first chunk - nothing lies in front of it, a distance beyond its text is invalid.
// kWrite false: the text is counted only; the span ends at the first block boundary that is a later chunk's start (starts[],
//   chunks chunk + 1 ..; those passed are counted as refuted) or with the final block.
// kWrite true: the span ends at stop_bit (kNoStart: with the final block) and must give text_n symbols, which go through
//   the ring to sym[0 .. text_n).
template <bool kWrite>
__device__ __forceinline__ GzipSpan inflate_span(Lds& T, uint16_t* ring, const uint8_t* comp, uint64_t end, uint64_t start_bit, bool first,
                                                 const uint64_t* starts, uint32_t n_chunks, uint32_t chunk, uint64_t stop_bit,
                                                 uint64_t text_n, uint16_t* sym) {
    constexpr uint32_t M = kRing - 1;
    const uint32_t lane = lane_id();
    const uint64_t limit = 8ull * end;
    Bits r;
    r.start(comp, end, start_bit);
    uint64_t pos = 0, flushed = 0;
    uint32_t next = chunk + 1, refuted = 0, status = 2;
    bool bad = false, last = false;
    const uint32_t a0 = kWrite ? (uint32_t)(((uintptr_t)sym >> 1) & 7u) : 0u;       // sym + p is 16-byte aligned where (a0 + p) % 8 == 0
    // symbols [flushed, upto) from the ring to global memory: single ones up to a 16-byte boundary, then 8 at a time
    auto flush = [&](uint64_t upto) {
        const uint32_t head = (uint32_t)min((uint64_t)((8u - ((a0 + (uint32_t)flushed) & 7u)) & 7u), upto - flushed);
        if (lane < head) sym[flushed + lane] = ring[(uint32_t)(flushed + lane) & M];
        flushed += head;
        const uint64_t n_vec = (upto - flushed) >> 3;
        for (uint64_t v = lane; v < n_vec; v += kWave) {
            const uint32_t q = (uint32_t)(flushed + 8 * v);
            uint32_t w[4];
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) w[e] = (uint32_t)ring[(q + 2 * e) & M] | (uint32_t)ring[(q + 2 * e + 1) & M] << 16;
            *(uint4*)(sym + flushed + 8 * v) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        flushed += 8 * n_vec;
        const uint32_t tail = (uint32_t)(upto - flushed);
        if (lane < tail) sym[flushed + lane] = ring[(uint32_t)(flushed + lane) & M];
        flushed = upto;
    };
    if (kWrite) {
        for (uint32_t e = lane; e < kRing; e += kWave) ring[e] = (uint16_t)(0x8000u | e);
    }
    __syncthreads();
    for (bool begun = false; !bad; begun = true) {
        if (begun) {                                                // a block boundary
            if (last) { status = 1; break; }
            const uint64_t p = r.consumed();
            if (kWrite) {
                if (p == stop_bit) { status = 0; break; }
            } else {
                while (next < n_chunks) {
                    const uint64_t s = starts[next];
                    if (s != kNoStart && s >= p) break;
                    refuted += s != kNoStart;
                    ++next;
                }
                if (next < n_chunks && starts[next] == p) { status = 0; break; }
            }
        }
        r.refill();
        last = r.take(1) != 0;
        const uint32_t type = r.take(2);
        if (type == 0) {                                            // stored
            const uint64_t p = (r.consumed() + 7) >> 3;             // (the rest of the byte is dropped)
            if (p + 4 > end) { bad = true; break; }
            r.in.seek(p);
            const uint32_t ln = r.in.fetch32(p);
            const uint32_t len = ln & 0xFFFFu;
            if ((ln >> 16) != (~len & 0xFFFFu) || p + 4 + len > end) { bad = true; break; }
            if (kWrite) {
                if (pos + len > text_n) { bad = true; break; }
                for (uint32_t done = 0; done < len;) {
                    const uint32_t piece = min(len - done, 4096u);
                    for (uint32_t j = lane; j < piece; j += kWave) ring[(uint32_t)(pos + j) & M] = comp[p + 4 + done + j];
                    pos += piece;
                    done += piece;
                    if (pos - flushed >= kFlushAt) flush(pos - ((a0 + (uint32_t)pos) & 7u));
                }
            } else {
                pos += len;
            }
            r.restart(p + 4 + len);
            continue;
        }
        if (type == 3) { bad = true; break; }
        if (type == 1) {
            build_fixed(T);
        } else if (!read_dynamic(r, T, limit)) {
            bad = true;
            break;
        }
        for (;;) {                                                  // the block's symbols
            r.refill();
            uint32_t e = uni(T.lut_ll[(uint32_t)r.bb & ((1u << kLitBits) - 1u)]);
            if (e == 0) e = uni(decode_canonical(T.cnt_ll, T.sym_ll, (uint32_t)r.bb, 15));
            if (e == 0) { bad = true; break; }
            r.take(e >> 9);
            const uint32_t s = e & 511u;
            if (s < 256) {
                if (kWrite) {
                    if (pos >= text_n) { bad = true; break; }
                    if (lane == 0) ring[(uint32_t)pos & M] = (uint16_t)s;
                }
                ++pos;
            } else if (s == 256) {
                break;
            } else if (s <= 285) {
                const uint32_t k = s - 257;
                const uint32_t length = kLenBase[k] + r.take(kLenExtra[k]);
                r.refill();
                uint32_t d = uni(T.lut_d[(uint32_t)r.bb & ((1u << kDistBits) - 1u)]);
                if (d == 0) d = uni(decode_canonical(T.cnt_d, T.sym_d, (uint32_t)r.bb, 15));
                if (d == 0 || (d & 511u) >= 30) { bad = true; break; }
                r.take(d >> 9);
                const uint32_t dk = d & 511u;
                const uint32_t dist = kDistBase[dk] + r.take(kDistExtra[dk]);
                if (first && dist > pos) { bad = true; break; }
                if (kWrite) {
                    if (pos + length > text_n) { bad = true; break; }
                    const uint32_t from = (uint32_t)pos + kRing - dist, to = (uint32_t)pos;
                    if (dist >= length) {
                        for (uint32_t j = lane; j < length; j += kWave) ring[(to + j) & M] = ring[(from + j) & M];
                    } else {
                        for (uint32_t j = lane; j < length; j += kWave) ring[(to + j) & M] = ring[(from + j % dist) & M];
                    }
                }
                pos += length;
            } else {
                bad = true;
                break;
            }
            if (r.consumed() > limit) { bad = true; break; }
            if (kWrite && pos - flushed >= kFlushAt) flush(pos - ((a0 + (uint32_t)pos) & 7u));
        }
        if (r.consumed() > limit) bad = true;
    }
    if (bad) status = 2;
    if (kWrite && status != 2) flush(pos);
    GzipSpan o;
    o.end_bit = r.consumed();
    o.text = pos;
    o.next = next;
    o.status = status;
    o.refuted = refuted;
    o.pad = 0;
    return o;
}

}  // namespace

}  // namespace rala_hip
