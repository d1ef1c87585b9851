// What the speculative gzip inflater (inflate_kernels.hip) and the host that drives it (ingest_gzip.hip) hand each other: plain
// structs, no device header - the host's chain builder (ingest_formats.h) compiles without one.
#pragma once

#include <stdint.h>

namespace rala_hip {

constexpr uint64_t kGzipNoStart = ~0ull;
constexpr uint64_t kGzipHeadReach = 1u << 20;       // a header (name, comment, extra field) longer than this is the host reader's
// what the counting pass found from one chunk's start: status 0 = it ended at the start of chunk `next`, 1 = its final block
// ended at bit end_bit, 2 = invalid, 3 = the chunk has no start; text = the bytes it gives; refuted = later starts it passed
struct GzipSpan {
    uint64_t end_bit, text;
    uint32_t next, status, refuted, pad;
};
// one true chunk for the writing pass: decoded from start_bit to the block boundary stop_bit (kGzipNoStart: to the final block's
// end), its text_n symbols to sym + text_off; first != 0: a member's first chunk (nothing lies in front of its text)
struct GzipJob {
    uint64_t start_bit, stop_bit, text_off, text_n;
    uint32_t first, pad;
};
// a member header the device found (gzip_member_find_kernel): the header's first byte, the bit its deflate bytes begin at, and
// the 8 bytes in front of the header - the trailer of a member that ends there (zeros where the file has no such bytes)
struct GzipMemberCand {
    uint64_t header_off, deflate_bit;
    uint32_t prev_crc, prev_isize;
};
// one member of the chain: its text, the CRC32 its trailer names, where that trailer lies in the file
struct GzipMember {
    uint64_t text_off, text_n, trailer_off;
    uint32_t crc, pad;
};
// a piece of the text whose CRC register gzip_piece_crc_kernel computes: n <= gzip_segment_bytes() bytes at text + off
struct GzipPiece {
    uint64_t off;
    uint32_t n, pad;
};

}  // namespace rala_hip
