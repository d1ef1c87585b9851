// What the speculative gzip inflater (inflate_kernels.hip) and the host that drives it (ingest_gzip.hip) hand each other: plain
// structs, no device header - the host's chain builder (ingest_formats.h) compiles without one.
#pragma once

#include <stdint.h>

namespace rala_hip {

constexpr uint64_t kGzipNoStart = ~0ull;
// what the counting pass found from one chunk's start: status 0 = it ended at the start of chunk `next`, 1 = its final block
// ended at bit end_bit, 2 = invalid, 3 = the chunk has no start; text = the bytes it gives; refuted = later starts it passed
struct GzipSpan {
    uint64_t end_bit, text;
    uint32_t next, status, refuted, pad;
};
// one true chunk for the writing pass: decoded from start_bit to the block boundary stop_bit (kGzipNoStart: to the final block's
// end), its text_n symbols to sym + text_off; first != 0: the stream's first chunk (nothing lies in front of its text)
struct GzipJob {
    uint64_t start_bit, stop_bit, text_off, text_n;
    uint32_t first, pad;
};

}  // namespace rala_hip
