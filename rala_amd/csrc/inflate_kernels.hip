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
#include <hip/hip_runtime.h>

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

}  // namespace

void launch_bgzf_inflate(const uint8_t* comp, const BgzfJob* jobs, uint32_t n_jobs, uint8_t* text, uint64_t text_cap, uint32_t* flags,
                         hipStream_t s) {
    if (n_jobs) hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(n_jobs), dim3(kWave), 0, s, comp, jobs, text, text_cap, flags);
}

}  // namespace rala_hip
