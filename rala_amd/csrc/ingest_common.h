// What the files of the device ingest share (ingest.hip: overlap text -> columns; ingest_ship.hip: a file's bytes to device
// memory; ingest_bgzf.hip, ingest_gzip.hip: compressed files -> text; ingest_sequences.hip: read files -> index and bases).
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "ctx_check.h"
#include "ingest_formats.h"
#include "kernels.h"
#include "orchestration.h"      // now_ms, trace_on
#include "stages.h"

namespace rala_hip {
namespace ingest {

constexpr size_t kBlockBytes = 32u << 20;       // one staging block

struct Fd {                                         // (closed on every way out - ADVICE round 4)
    int fd = -1;
    ~Fd() { if (fd >= 0) close(fd); }
};

// the file opened for reading, its size; what is no regular file (a directory; a FIFO, its writer not waited for) is refused
inline int open_regular(rala_hip_ctx* ctx, const char* path, Fd& file, uint64_t* size) {
    file.fd = open(path, O_RDONLY | O_NONBLOCK);
    if (file.fd < 0) return fail(ctx, RALA_HIP_EINVAL, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(file.fd, &st) != 0 || !S_ISREG(st.st_mode)) return fail(ctx, RALA_HIP_ENOTAFILE, std::string("not a regular file: ") + path);
    *size = (uint64_t)st.st_size;
    return RALA_HIP_OK;
}

// what every way into the tokeniser needs of the context first
inline int ingest_ready(rala_hip_ctx* ctx, bool mhap) {
    if (ctx->n_reads == 0) return fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (ctx->n_name_buckets == 0 && !mhap) return fail(ctx, RALA_HIP_EINVAL, "no name table set (rala_hip_set_name_table)");
    return RALA_HIP_OK;
}

// The window a file's text goes through device memory in: the caller's option, or (0) a quarter of what is free, at least 256 MB.
inline uint64_t text_window_bytes(uint64_t option) {
    if (option) return option;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    return std::max<uint64_t>(256ull << 20, free_b / 4);
}

// ---- ingest_ship.hip -----------------------------------------------------------------------------------------------
// The ship stage: bytes [off, off + len) of the file to dev (null: read only) by reader threads - two pinned staging blocks
// each, a block's copy queued behind its read; scan (optional) sees every block in host memory as it was read.  meanwhile
// runs on the calling thread while the readers work (false: out of device memory).  0 ok, 1 a read / copy failed, 2 meanwhile failed.
using BlockScan = std::function<void(uint64_t block, const uint8_t* bytes, size_t n)>;
int ship_file(int fd, uint64_t off, uint64_t len, uint8_t* dev, int device, uint32_t threads, const BlockScan* scan,
              const std::function<bool()>& meanwhile, uint32_t* n_readers_out);

// ---- ingest_bgzf.hip -----------------------------------------------------------------------------------------------
// A BGZF file on the device: the members indexed while the file is read once (every reader thread scans its staging blocks
// for member headers; the chain is walked from offset 0 after the join), the compressed bytes kept in device memory when
// they fit the window (else shipped window by window: the members that cover it), the members inflated into the text buffer.
struct BgzfFile {
    int fd = -1;                        // (the caller's)
    uint64_t file_n = 0, text_n = 0;
    std::vector<BgzfMember> jobs;       // the members with text, in file order
    uint64_t n_members = 0;
    bool resident = false;              // all compressed bytes in ctx->d_bgzf_comp
    uint64_t comp_origin = 0;           // resident: the file offset of ctx->d_bgzf_comp's first byte (a piece: its range's)
    float ship_ms = 0, inflate_ms = 0;
    uint64_t shipped = 0;
    uint32_t n_readers = 0;
};
// index the open file of file_n bytes (and ship it when it fits); *valid = false: not a chain of members the host reader takes
int bgzf_open(rala_hip_ctx* ctx, int fd, uint64_t file_n, const char* path, uint32_t threads, uint64_t window, BgzfFile& f, bool* valid);
// A PIECE of the file instead (ingest_formats.h: the members whose header begins in bytes [lo, hi), bgzf_walk_range), indexed
// and shipped without reading anything in front of lo: the range goes to ctx->d_bgzf_comp through the readers, who scan it;
// what the piece's last member and the members behind it hold of the next `follow_text` bytes of text (the first byte behind
// the piece's own text decides who owns the line there, the tokeniser's halo follows) is read header by header and copied
// behind it.  f then describes the piece alone: resident, text offsets from its first member, text_n = own_text + what follows.
// *valid = false: the chain broke, in the piece or in what follows it (piece->begin / end say where it stood).
int bgzf_open_piece(rala_hip_ctx* ctx, int fd, uint64_t file_n, const char* path, uint32_t threads, uint64_t lo, uint64_t hi,
                    uint64_t follow_text, BgzfFile& f, BgzfPiece* piece, uint64_t* own_text, bool* valid);
// The text [lo, lo + n_avail) of a BGZF file (and the byte in front of it) in device memory: the members that cover it
// shipped (unless the file is resident) and inflated into ctx->d_paf_text, `pad` in the bytes behind the text up to cap.
// meanwhile runs while the readers work (false: `room` could not be made).  out->flag != 0: the inflater refused a member
// (the text's memory is given back).  t0 .. t_ship: the ship; t1: the text was there.
struct TextArrival {
    uint8_t* text = nullptr;
    uint32_t flag = 0;
    double t0 = 0, t_ship = 0, t1 = 0;
};
int bgzf_text_range(rala_hip_ctx* ctx, BgzfFile& f, uint64_t lo, uint64_t n_avail, uint64_t cap, int pad, uint32_t threads,
                    const std::function<bool()>& meanwhile, const char* room, TextArrival* out);

// ---- ingest_gzip.hip -----------------------------------------------------------------------------------------------
// A gzip file (one member; with the option gzip_members any number of them) whose compressed bytes lie in ctx->d_bgzf_comp, the
// chain of its true chunks and its members.
struct GzipStream {
    std::vector<GzipJob> chain;             // the true chunks, text offsets from the text's start
    std::vector<GzipMember> members;        // text range, trailer and CRC32 of every member (one: the whole text)
    std::vector<uint64_t> job_floor;        // per job of the chain: where its member's text begins
    uint64_t file_n = 0, end = 0, text_n = 0;       // file_n: set by the caller
    uint32_t crc = 0;                       // the last trailer's
    // the proof per member: the registers and lengths of the pieces of members[proven]'s text seen so far, and the verdict
    size_t proven = 0;
    std::vector<uint32_t> reg;
    std::vector<uint64_t> len;
    bool crc_ok = true;
    uint64_t n_cands = 0;                   // member headers the device found (false ones included)
    float member_find_ms = 0;
    float ship_ms = 0;
    uint32_t n_readers = 0;
    rala_hip_gzip_timings tm = {};
};
// The whole text at once (overlap files), left in ctx->d_gzip_text with newlines behind it.  *valid = false: not proven.
int gzip_inflate(rala_hip_ctx* ctx, int fd, const char* path, uint32_t threads, GzipStream& g, bool* valid);
// The text WINDOW by window (read files).
struct GzipWalk : GzipStream {
    uint64_t window = 0;                    // text bytes a window holds at most (at least the largest chunk's)
    size_t next_job = 0;
    uint64_t windows = 0;
};
// chain, members: null, or those of an earlier walk taken over (refused where a member's trailer is no longer what it was)
int gzip_walk_open(rala_hip_ctx* ctx, int fd, const char* path, uint32_t threads, uint64_t want_window, uint64_t front, uint64_t behind,
                   const std::vector<GzipJob>* chain, const std::vector<GzipMember>* members, GzipWalk& g, bool* valid);
int gzip_walk_next(rala_hip_ctx* ctx, GzipWalk& g, uint8_t* text, uint64_t* lo, uint64_t* n, uint32_t* flag);
bool gzip_walk_proven(const GzipWalk& g);
// the trace line of either driver (windows = 0: the whole text at once)
void trace_gzip(const GzipStream& g, uint64_t windows, uint64_t window);

}  // namespace ingest
}  // namespace rala_hip
