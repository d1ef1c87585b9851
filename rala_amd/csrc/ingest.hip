// Host side of the device tokeniser (ingest_kernels.hip): the file's text to device memory - reader threads with pinned
// staging blocks of their own, every block's copy queued behind its read, so that the disk / page cache and PCIe work at the
// same time - then count, scan, parse, and the columns become the context's overlaps (rala_hip_set_overlaps, device memory).
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kernels.h"
#include "name_table.h"
#include "stages.h"

using namespace rala_hip;

namespace {

constexpr size_t kBlockBytes = 32u << 20;       // one staging block
constexpr uint32_t kMaxReaders = 8;        // (measured at C3: 4 readers 107 ms, 8: 70 - 73 ms, 12 - 16: 85 - 130 ms on the 16 CPUs a box allows)

// Pinned staging blocks are expensive to make (the pages are locked one by one) and cheap to keep: a pool of the
// process, two blocks per reader.
struct StagingPool {
    std::mutex m;
    std::vector<void*> free_blocks;
    // (never freed: at process exit the runtime may be gone before this object is, and the memory goes with the process)
    void* take() {
        {
            std::lock_guard<std::mutex> hold(m);
            if (!free_blocks.empty()) { void* p = free_blocks.back(); free_blocks.pop_back(); return p; }
        }
        void* p = nullptr;
        return hipHostMalloc(&p, kBlockBytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
    }
    void give(void* p) {
        std::lock_guard<std::mutex> hold(m);
        free_blocks.push_back(p);
    }
};
StagingPool& staging() {
    static StagingPool pool;
    return pool;
}

int ingest_fail(rala_hip_ctx* ctx, int code, const std::string& msg) {
    ctx->err = msg;
    return code;
}

#define INGEST_CHECK(call)                                                                                  \
    do {                                                                                                    \
        const hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                             \
            return ingest_fail(ctx, e_ == hipErrorOutOfMemory ? RALA_HIP_ENOMEM : RALA_HIP_EDEVICE,         \
                               std::string(#call) + ": " + hipGetErrorString(e_));                          \
        }                                                                                                   \
    } while (0)

struct Fd {                                         // (closed on every way out - ADVICE round 4)
    int fd = -1;
    ~Fd() { if (fd >= 0) close(fd); }
};

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The ship stage: bytes [off, off + len) of the file to dev (null: read only) by reader threads - two pinned staging blocks
// each, a block's copy queued behind its read; scan (optional) sees every block in host memory as it was read.  meanwhile
// runs on the calling thread while the readers work (false: out of device memory).  0 ok, 1 a read / copy failed, 2 meanwhile failed.
using BlockScan = std::function<void(uint64_t block, const uint8_t* bytes, size_t n)>;
int ship_file(int fd, uint64_t off, uint64_t len, uint8_t* dev, int device, uint32_t threads, const BlockScan* scan,
              const std::function<bool()>& meanwhile, uint32_t* n_readers_out) {
    const uint64_t n_blocks = (len + kBlockBytes - 1) / kBlockBytes;
    const uint32_t n_readers = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(threads ? threads : 1, kMaxReaders), n_blocks));
    if (n_readers_out) *n_readers_out = n_readers;
    std::atomic<uint64_t> next(0);
    std::atomic<int> failed(0);
    std::vector<std::thread> readers;
    for (uint32_t t = 0; t < n_readers && n_blocks; ++t) {
        readers.emplace_back([&]() {
            if (hipSetDevice(device) != hipSuccess) { failed = 1; return; }
            hipStream_t cs = nullptr;
            hipEvent_t ev[2] = {nullptr, nullptr};
            void* blk[2] = {staging().take(), staging().take()};
            bool ok = blk[0] && blk[1] && hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) == hipSuccess &&
                      hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) == hipSuccess &&
                      hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) == hipSuccess;
            bool busy[2] = {false, false};
            for (int k = 0; ok && !failed; k ^= 1) {
                const uint64_t b = next.fetch_add(1);
                if (b >= n_blocks) break;
                if (busy[k]) ok = hipEventSynchronize(ev[k]) == hipSuccess;       // the block's last copy has left it
                const uint64_t o = b * kBlockBytes;
                const size_t n = (size_t)std::min<uint64_t>(kBlockBytes, len - o);
                size_t got = 0;
                while (ok && got < n) {
                    const ssize_t r = pread(fd, (char*)blk[k] + got, n - got, (off_t)(off + o + got));
                    if (r <= 0) { ok = false; break; }
                    got += (size_t)r;
                }
                if (ok && dev) {
                    ok = hipMemcpyAsync(dev + o, blk[k], n, hipMemcpyHostToDevice, cs) == hipSuccess && hipEventRecord(ev[k], cs) == hipSuccess;
                    busy[k] = ok;
                }
                if (ok && scan) (*scan)(b, (const uint8_t*)blk[k], n);     // (reads the block while it is copied)
            }
            if (cs) ok = (hipStreamSynchronize(cs) == hipSuccess) && ok;
            if (!ok) failed = 1;
            for (int k = 0; k < 2; ++k) {
                if (ev[k]) (void)hipEventDestroy(ev[k]);
                if (blk[k]) staging().give(blk[k]);
            }
            if (cs) (void)hipStreamDestroy(cs);
        });
    }
    const bool room = meanwhile();
    for (auto& th : readers) th.join();
    return !room ? 2 : failed ? 1 : 0;
}

// The device memory the tokeniser will want for n bytes of text (made while the readers work: hipMalloc of a few hundred
// megabytes takes a millisecond and more, eight columns of them 4 - 9 ms - behind the copies that is free).  The number of
// records is not known yet: a record has at least 23 bytes, files in the wild 60 - 150 per line; room for one per 32 bytes
// is made now (twice what a synthetic file needs) and the exact count decides later whether that was enough.
bool tokeniser_memory(rala_hip_ctx* ctx, uint64_t n, uint64_t n_chunks, size_t extra_rows, const PafTarget& T) {
    const size_t guess = (size_t)(n / 32) + 1024 + extra_rows;
    bool ok = true;
    for (int k = 0; k < 7 && ok; ++k) ok = T.col[k]->ensure(guess) == hipSuccess;
    ok = ok && T.strand->ensure(guess) == hipSuccess && ctx->d_paf_bad.ensure(2) == hipSuccess;
    if (n_chunks) {
        ok = ok && ctx->d_paf_chunk[0].ensure(n_chunks + 2) == hipSuccess && ctx->d_paf_chunk[1].ensure(n_chunks + 2) == hipSuccess &&
             ctx->d_scan_ws.ensure(scan_workspace_bytes(std::max<uint64_t>(std::max<uint64_t>(n_chunks, ctx->n_reads), ctx->n_ovl) + 2)) == hipSuccess;
    }
    return ok;
}

// What follows once the text is in device memory, for the plain file and the BGZF one alike: count, scan, parse into T's
// columns (n, n_avail, first_is_start: launch_paf_count / launch_paf_parse), then the text's memory back.  t1: when the
// text was there; ship_ms = t1 - t0.
int tokenise_text(rala_hip_ctx* ctx, const uint8_t* text, uint64_t n, uint64_t n_avail, bool first_is_start, bool check_lengths,
                  size_t extra_rows, const PafTarget& T, PafRange* out, double t0, double t1, uint32_t n_readers) {
    hipStream_t s = ctx->stream;
    const uint32_t chunk = paf_chunk_bytes();
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    const bool trace = getenv("RALA_HIP_TRACE") != nullptr;
    double tc = t1, tp0 = t1, tp1 = t1;
    uint32_t n_lines = 0;
    if (n_chunks) {
        launch_paf_count(text, n, first_is_start, ctx->d_paf_chunk[0].p, s);
        launch_exclusive_scan(ctx->d_paf_chunk[0].p, ctx->d_paf_chunk[1].p, n_chunks, ctx->d_scan_ws.p, s);
        INGEST_CHECK(hipMemcpyAsync(&n_lines, ctx->d_paf_chunk[1].p + n_chunks, 4, hipMemcpyDeviceToHost, s));
        INGEST_CHECK(hipStreamSynchronize(s));
    }
    tc = now_ms();
    if ((uint64_t)n_lines >= 0xFFFFFFF0ull / 2) return ingest_fail(ctx, RALA_HIP_ETOOLARGE, "too many overlaps for 32-bit bound offsets");
    for (int k = 0; k < 7; ++k) INGEST_CHECK(T.col[k]->ensure((size_t)n_lines + 1 + extra_rows));
    INGEST_CHECK(T.strand->ensure((size_t)n_lines + 1 + extra_rows));
    unsigned long long bad = ~0ull;
    uint32_t flags = 0;
    if (n_lines) {
        tp0 = now_ms();
        INGEST_CHECK(hipMemsetAsync(ctx->d_paf_bad.p, 0xFF, 8, s));
        INGEST_CHECK(hipMemsetAsync(ctx->d_paf_bad.p + 1, 0, 8, s));
        PafColumns cols;
        cols.a_id = T.col[0]->p; cols.b_id = T.col[1]->p; cols.a_begin = T.col[2]->p; cols.a_end = T.col[3]->p;
        cols.b_begin = T.col[4]->p; cols.b_end = T.col[5]->p; cols.length = T.col[6]->p; cols.strand = T.strand->p;
        launch_paf_parse(text, n, n_avail, first_is_start, ctx->d_paf_chunk[1].p, ctx->d_name_buckets.p, std::max<uint64_t>(ctx->n_name_buckets, 1),
                         (const char*)ctx->d_name_arena.p, ctx->d_read_len.p, (uint32_t)ctx->n_reads, check_lengths, cols,
                         (uint32_t*)(ctx->d_paf_bad.p + 1), ctx->d_paf_bad.p, s, T.mhap);
        unsigned long long back[2] = {0, 0};
        INGEST_CHECK(hipMemcpyAsync(back, ctx->d_paf_bad.p, 16, hipMemcpyDeviceToHost, s));
        INGEST_CHECK(hipStreamSynchronize(s));
        INGEST_CHECK(hipGetLastError());
        bad = back[0];
        flags = (uint32_t)back[1];
        tp1 = now_ms();
    }
    ctx->d_paf_text.release();                  // (the text is as large as the file: not kept)
    const double t2 = now_ms();
    ctx->ingest_tm.ship_ms = (float)(t1 - t0);
    ctx->ingest_tm.tokenize_ms = (float)(t2 - t1);
    ctx->ingest_tm.bytes = n;
    ctx->ingest_tm.lines = n_lines;
    if (trace) {
        fprintf(stderr, "[trace] device ingest: %.2f GB of text shipped in %.1f ms by %u readers, %u lines tokenised in %.2f ms (count + scan %.2f, "
                "columns' memory %.2f, parse %.2f, the text's memory back %.2f; flags %u)\n",
                n / 1e9, t1 - t0, n_readers, n_lines, t2 - t1, tc - t1, tp0 - tc, tp1 - tp0, t2 - tp1, flags);
    }
    out->n_lines = n_lines;
    out->first_bad = bad;
    out->flags = flags;
    return RALA_HIP_OK;
}

}  // namespace

// The lines that START in bytes [lo, hi) of the file (hi = ~0: to its end), tokenised on the device into `T`'s columns (room for
// extra_rows more rows than the range holds: a rank of a sharded run receives the heads of its neighbours' first runs).  The
// text is shipped by reader threads - two pinned staging blocks each, a block's copy queued behind its read - with what the last
// lines' first eleven columns may need behind hi.
int rala_hip::paf_tokenise_range(rala_hip_ctx* ctx, const char* path, uint64_t lo, uint64_t hi, bool check_lengths, uint32_t threads,
                                 size_t extra_rows, const PafTarget& T, PafRange* out) {
    if (!ctx || !path || !out) return RALA_HIP_EINVAL;
    *out = PafRange();
    if (ctx->n_reads == 0) return ingest_fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (ctx->n_name_buckets == 0 && !T.mhap) return ingest_fail(ctx, RALA_HIP_EINVAL, "no name table set (rala_hip_set_name_table)");
    INGEST_CHECK(hipSetDevice(ctx->device));
    Fd file;
    file.fd = open(path, O_RDONLY);
    const int fd = file.fd;
    if (fd < 0) return ingest_fail(ctx, RALA_HIP_EINVAL, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return ingest_fail(ctx, RALA_HIP_ENOTAFILE, std::string("not a regular file: ") + path);
    const uint64_t file_n = (uint64_t)st.st_size;
    hi = std::min(hi, file_n);
    lo = std::min(lo, hi);
    const uint64_t n = hi - lo;                                             // bytes whose line starts are ours
    const uint64_t n_avail = std::min<uint64_t>(file_n - lo, n + paf_halo_bytes());
    bool first_is_start = lo == 0;
    if (lo) {
        char before = 0;
        if (pread(fd, &before, 1, (off_t)(lo - 1)) != 1) return ingest_fail(ctx, RALA_HIP_EDEVICE, std::string("reading ") + path + " failed");
        first_is_start = before == '\n';
    }
    const uint32_t chunk = paf_chunk_bytes();
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    if (n_chunks >= 0xFFFFFFF0ull) return ingest_fail(ctx, RALA_HIP_ETOOLARGE, "file too large for 32-bit chunk ids");
    const uint64_t cap = n_chunks * chunk + 4096 + 64;
    hipStream_t s = ctx->stream;
    const double t0 = now_ms();
    if (ctx->d_paf_text.ensure(cap) != hipSuccess) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the file's text");
    // what lies behind the text reads as newlines
    INGEST_CHECK(hipMemsetAsync(ctx->d_paf_text.p + n_avail, '\n', cap - n_avail, s));
    uint32_t n_readers = 0;
    const int shipped = ship_file(fd, lo, n_avail, ctx->d_paf_text.p, ctx->device, threads, nullptr,
                                  [&]() { return tokeniser_memory(ctx, n, n_chunks, extra_rows, T); }, &n_readers);
    if (shipped == 2) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the overlap columns");
    if (shipped) return ingest_fail(ctx, RALA_HIP_EDEVICE, std::string("reading / copying ") + path + " failed");
    INGEST_CHECK(hipStreamSynchronize(s));
    const double t1 = now_ms();
    out->file_bytes = file_n;
    return tokenise_text(ctx, ctx->d_paf_text.p, n, n_avail, first_is_start, check_lengths, extra_rows, T, out, t0, t1, n_readers);
}

// ---- BGZF: the member index -------------------------------------------------------------------
namespace {

constexpr uint64_t kHeaderReach = 12 + 65535;      // the bytes a member header may occupy (XLEN < 2^16)

struct BgzfCand {
    uint64_t pos;
    uint32_t bsize;         // the member's bytes (BSIZE + 1); 0: no member header the host reader would take
    uint32_t hdr;           // 12 + XLEN
    uint32_t prev_isize;    // the 4 bytes in front of pos (the ISIZE of a member that ends here)
};
struct BgzfMember {
    uint64_t off, text_off;
    uint32_t bsize, hdr, isize;
};

// is_bgzf of the host reader (io.cpp, BgzfSource): the first 18 bytes
bool bgzf_head(const uint8_t* h, uint64_t n) {
    return n >= 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) != 0 && h[10] == 6 && h[11] == 0 && h[12] == 'B' &&
           h[13] == 'C' && h[14] == 2 && h[15] == 0;
}

// The member-header candidates among the bytes [off, off + n) of a file of file_n bytes: at(q) gives byte q for q in
// [off - min(off, 8), min(file_n, off + n + kHeaderReach)).  A candidate is every 0x1f 0x8b 0x08 with FEXTRA; its BSIZE
// is read as read_block reads it (BgzfSource: any XLEN, the last "BC" subfield of length 2, bsize >= 12 + XLEN + 8).
template <class At>
void bgzf_scan(const uint8_t* bytes, uint64_t n, uint64_t off, uint64_t file_n, const At& at, std::vector<BgzfCand>& out) {
    const uint8_t* const end = bytes + n;
    for (const uint8_t* h = (const uint8_t*)memchr(bytes, 0x1f, n); h; h = (const uint8_t*)memchr(h + 1, 0x1f, (size_t)(end - h - 1))) {
        const uint64_t q = off + (uint64_t)(h - bytes);
        if (q + 12 > file_n) break;
        if (at(q + 1) != 0x8b || at(q + 2) != 8 || !(at(q + 3) & 4)) {
            if (h + 1 >= end) break;
            continue;
        }
        BgzfCand c;
        c.pos = q;
        c.bsize = 0;
        c.prev_isize = 0;
        if (q >= 4) for (int k = 3; k >= 0; --k) c.prev_isize = (c.prev_isize << 8) | at(q - 4 + (uint64_t)k);
        const uint32_t xlen = at(q + 10) | (uint32_t)at(q + 11) << 8;
        c.hdr = 12 + xlen;
        if (q + 12 + xlen <= file_n) {
            uint32_t bsize = 0;
            for (uint32_t k = 0; k + 4 <= xlen;) {
                const uint64_t e = q + 12 + k;
                const uint32_t slen = at(e + 2) | (uint32_t)at(e + 3) << 8;
                if (at(e) == 'B' && at(e + 1) == 'C' && slen == 2 && k + 6 <= xlen) bsize = (at(e + 4) | (uint32_t)at(e + 5) << 8) + 1;
                k += 4 + slen;
            }
            if (bsize >= 12 + xlen + 8) c.bsize = bsize;
        }
        out.push_back(c);
        if (h + 1 >= end) break;
    }
}

// The chain of members from offset 0 through the candidates (in file order); tail: the file's last 4 bytes (the last member's
// ISIZE).  false: the chain breaks - a position with no member header, a member beyond the end, ISIZE > 65536.
bool bgzf_walk(const std::vector<std::vector<BgzfCand>>& blocks, uint64_t file_n, uint32_t tail, std::vector<BgzfMember>& members) {
    members.clear();
    uint64_t o = 0;
    size_t b = 0, i = 0;
    while (o < file_n) {
        while (b < blocks.size() && (i >= blocks[b].size() || blocks[b][i].pos < o)) {
            if (i >= blocks[b].size()) { ++b; i = 0; } else { ++i; }
        }
        if (b >= blocks.size()) return false;
        const BgzfCand& c = blocks[b][i];
        if (c.pos != o || c.bsize == 0 || o + c.bsize > file_n) return false;
        if (!members.empty()) members.back().isize = c.prev_isize;
        BgzfMember m;
        m.off = o; m.bsize = c.bsize; m.hdr = c.hdr; m.isize = 0; m.text_off = 0;
        members.push_back(m);
        o += c.bsize;
    }
    if (!members.empty()) members.back().isize = tail;
    uint64_t t = 0;
    for (BgzfMember& m : members) {
        if (m.isize > 65536) return false;
        m.text_off = t;
        t += m.isize;
    }
    return true;
}

uint32_t le32(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the index of a file in memory, scanned in blocks of block_bytes (what the readers do with their staging blocks)
bool bgzf_index_bytes(const uint8_t* bytes, uint64_t n, uint64_t block_bytes, std::vector<BgzfMember>& members) {
    if (!bgzf_head(bytes, n)) return false;
    const uint64_t n_blocks = (n + block_bytes - 1) / block_bytes;
    std::vector<std::vector<BgzfCand>> cand(n_blocks);
    auto at = [&](uint64_t q) { return bytes[q]; };
    for (uint64_t b = 0; b < n_blocks; ++b) {
        const uint64_t off = b * block_bytes;
        bgzf_scan(bytes + off, std::min(block_bytes, n - off), off, n, at, cand[b]);
    }
    return bgzf_walk(cand, n, le32(bytes + n - 4), members);
}

// A BGZF file on the device: the members indexed while the file is read once (every reader thread scans its staging blocks
// for member headers; the chain is walked from offset 0 after the join), the compressed bytes kept in device memory when
// they fit the window (else shipped window by window: the members that cover it), the members inflated into the text
// buffer, and from there on the plain file's way (tokenise_text).
struct BgzfFile {
    Fd file;
    uint64_t file_n = 0, text_n = 0;
    std::vector<BgzfMember> jobs;       // the members with text, in file order
    uint64_t n_members = 0;
    bool resident = false;              // all compressed bytes in ctx->d_bgzf_comp
    float ship_ms = 0, inflate_ms = 0;
    uint64_t shipped = 0;
    uint32_t n_readers = 0;
};

// index the file (and ship it when it fits); *valid = false: not a chain of members the host reader takes
int bgzf_open(rala_hip_ctx* ctx, const char* path, uint32_t threads, uint64_t window, BgzfFile& f, bool* valid) {
    *valid = false;
    f.file.fd = open(path, O_RDONLY);
    if (f.file.fd < 0) return ingest_fail(ctx, RALA_HIP_EINVAL, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(f.file.fd, &st) != 0 || !S_ISREG(st.st_mode)) return ingest_fail(ctx, RALA_HIP_ENOTAFILE, std::string("not a regular file: ") + path);
    f.file_n = (uint64_t)st.st_size;
    if (f.file_n < 18) return RALA_HIP_OK;
    const double t0 = now_ms();
    f.resident = f.file_n <= window;
    if (f.resident && ctx->d_bgzf_comp.ensure(f.file_n + 64) != hipSuccess) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
    const int fd = f.file.fd;
    const uint64_t file_n = f.file_n;
    const uint64_t n_blocks = (file_n + kBlockBytes - 1) / kBlockBytes;
    std::vector<std::vector<BgzfCand>> cand(n_blocks);
    std::atomic<int> edge_failed(0);
    const BlockScan scan = [&](uint64_t b, const uint8_t* bytes, size_t n) {
        // the block, the 8 bytes in front of it and what a header that starts in it may reach behind it
        const uint64_t off = b * kBlockBytes;
        uint8_t pre[8];
        const uint64_t n_pre = std::min<uint64_t>(8, off);
        std::vector<uint8_t> ext((size_t)std::min<uint64_t>(kHeaderReach, file_n - off - n));
        if ((n_pre && pread(fd, pre, n_pre, (off_t)(off - n_pre)) != (ssize_t)n_pre) ||
            (!ext.empty() && pread(fd, ext.data(), ext.size(), (off_t)(off + n)) != (ssize_t)ext.size())) {
            edge_failed = 1;
            return;
        }
        auto at = [&](uint64_t q) -> uint8_t {
            if (q < off) return pre[n_pre - (off - q)];
            if (q < off + n) return bytes[q - off];
            return ext[q - off - n];
        };
        bgzf_scan(bytes, n, off, file_n, at, cand[b]);
    };
    const int shipped = ship_file(fd, 0, file_n, f.resident ? ctx->d_bgzf_comp.p : nullptr, ctx->device, threads, &scan,
                                  []() { return true; }, &f.n_readers);
    if (shipped || edge_failed) return ingest_fail(ctx, RALA_HIP_EDEVICE, std::string("reading / copying ") + path + " failed");
    uint8_t tail[4];
    if (pread(fd, tail, 4, (off_t)(file_n - 4)) != 4) return ingest_fail(ctx, RALA_HIP_EDEVICE, std::string("reading ") + path + " failed");
    std::vector<BgzfMember> members;
    if (!bgzf_walk(cand, file_n, le32(tail), members)) return RALA_HIP_OK;
    f.n_members = members.size();
    for (const BgzfMember& m : members) {
        if (m.isize) f.jobs.push_back(m);
        f.text_n += m.isize;
    }
    f.shipped = f.resident ? file_n : 0;
    f.ship_ms = (float)(now_ms() - t0);
    *valid = true;
    return RALA_HIP_OK;
}

// The text [lo, lo + n_avail) of a BGZF file (and the byte in front of it) in device memory: the members that cover it
// shipped (unless the file is resident) and inflated into ctx->d_paf_text, `pad` in the bytes behind the text up to cap.
// meanwhile runs while the readers work (false: `room` could not be made).  out->flag != 0: the inflater refused a member
// (the text's memory is given back).
struct BgzfText {
    uint8_t* text = nullptr;
    uint32_t flag = 0;
    double t0 = 0, t_ship = 0, t1 = 0;
};
int bgzf_text_range(rala_hip_ctx* ctx, BgzfFile& f, uint64_t lo, uint64_t n_avail, uint64_t cap, int pad, uint32_t threads,
                    const std::function<bool()>& meanwhile, const char* room, BgzfText* out) {
    hipStream_t s = ctx->stream;
    // the members that hold the text [lo - 1, lo + n_avail) (the byte in front of lo says whether lo starts a line)
    const uint64_t need_lo = lo ? lo - 1 : 0, need_hi = lo + n_avail;
    size_t j0 = 0, j1 = 0;
    if (need_hi > need_lo) {
        auto by_text = [](const BgzfMember& m, uint64_t t) { return m.text_off < t; };
        j1 = std::lower_bound(f.jobs.begin(), f.jobs.end(), need_hi, by_text) - f.jobs.begin();
        j0 = std::lower_bound(f.jobs.begin(), f.jobs.end(), need_lo + 1, by_text) - f.jobs.begin() - 1;
    }
    const uint64_t base = j1 > j0 ? f.jobs[j0].text_off : lo;
    const uint64_t shift = lo - base;
    const uint64_t extent = j1 > j0 ? f.jobs[j1 - 1].text_off + f.jobs[j1 - 1].isize - base : 0;
    const uint64_t size = std::max(shift + cap, extent) + 64;
    out->t0 = now_ms();
    if (ctx->d_paf_text.ensure(size) != hipSuccess) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the file's text");
    uint64_t comp_base = 0;
    if (!f.resident && j1 > j0) {
        comp_base = f.jobs[j0].off;
        const uint64_t c_len = f.jobs[j1 - 1].off + f.jobs[j1 - 1].bsize - comp_base;
        if (ctx->d_bgzf_comp.ensure(c_len + 64) != hipSuccess) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
        const int shipped = ship_file(f.file.fd, comp_base, c_len, ctx->d_bgzf_comp.p, ctx->device, threads, nullptr, meanwhile, &f.n_readers);
        if (shipped == 2) return ingest_fail(ctx, RALA_HIP_ENOMEM, room);
        if (shipped) return ingest_fail(ctx, RALA_HIP_EDEVICE, "reading / copying the compressed file failed");
        f.shipped += c_len;
    } else if (!meanwhile()) {
        return ingest_fail(ctx, RALA_HIP_ENOMEM, room);
    }
    out->t_ship = now_ms();
    std::vector<BgzfJob> jobs(j1 - j0);
    for (size_t j = j0; j < j1; ++j) {
        const BgzfMember& m = f.jobs[j];
        BgzfJob& J = jobs[j - j0];
        J.comp_off = m.off + m.hdr - comp_base;
        J.text_off = m.text_off - base;
        J.deflate_len = m.bsize - m.hdr - 8;
        J.isize = m.isize;
    }
    uint32_t flag = 0;
    if (!jobs.empty()) {
        INGEST_CHECK(ctx->d_bgzf_jobs.ensure(jobs.size() * sizeof(BgzfJob)));
        INGEST_CHECK(ctx->d_bgzf_flag.ensure(1));
        INGEST_CHECK(hipMemcpyAsync(ctx->d_bgzf_jobs.p, jobs.data(), jobs.size() * sizeof(BgzfJob), hipMemcpyHostToDevice, s));
        INGEST_CHECK(hipMemsetAsync(ctx->d_bgzf_flag.p, 0, 4, s));
        launch_bgzf_inflate(ctx->d_bgzf_comp.p, (const BgzfJob*)ctx->d_bgzf_jobs.p, (uint32_t)jobs.size(), ctx->d_paf_text.p, size, ctx->d_bgzf_flag.p, s);
        INGEST_CHECK(hipGetLastError());
        INGEST_CHECK(hipMemcpyAsync(&flag, ctx->d_bgzf_flag.p, 4, hipMemcpyDeviceToHost, s));
    }
    uint8_t* const text = ctx->d_paf_text.p + shift;
    INGEST_CHECK(hipMemsetAsync(text + n_avail, pad, cap - n_avail, s));
    INGEST_CHECK(hipStreamSynchronize(s));
    out->t1 = now_ms();
    f.inflate_ms += (float)(out->t1 - out->t_ship);
    if (flag) ctx->d_paf_text.release();
    out->text = text;
    out->flag = flag;
    return RALA_HIP_OK;
}

// bgzf's paf_tokenise_range: the lines that start in bytes [lo, hi) of the file's TEXT
int bgzf_tokenise_range(rala_hip_ctx* ctx, BgzfFile& f, uint64_t lo, uint64_t hi, bool check_lengths, uint32_t threads, const PafTarget& T,
                        PafRange* out) {
    *out = PafRange();
    hi = std::min(hi, f.text_n);
    lo = std::min(lo, hi);
    const uint64_t n = hi - lo;
    const uint64_t n_avail = std::min<uint64_t>(f.text_n - lo, n + paf_halo_bytes());
    const uint32_t chunk = paf_chunk_bytes();
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    if (n_chunks >= 0xFFFFFFF0ull) return ingest_fail(ctx, RALA_HIP_ETOOLARGE, "file too large for 32-bit chunk ids");
    const uint64_t cap = n_chunks * chunk + 4096 + 64;
    // what lies behind the text reads as newlines (as for the plain file)
    BgzfText bt;
    const int rc = bgzf_text_range(ctx, f, lo, n_avail, cap, '\n', threads, [&]() { return tokeniser_memory(ctx, n, n_chunks, 0, T); },
                                   "device memory for the overlap columns", &bt);
    if (rc != RALA_HIP_OK) return rc;
    if (bt.flag) {
        out->flags = bt.flag;
        return RALA_HIP_OK;
    }
    const uint8_t* const text = bt.text;
    bool first_is_start = lo == 0;
    if (lo) {
        uint8_t before = 0;
        INGEST_CHECK(hipMemcpy(&before, text - 1, 1, hipMemcpyDeviceToHost));
        first_is_start = before == '\n';
    }
    out->file_bytes = f.file_n;
    return tokenise_text(ctx, text, n, n_avail, first_is_start, check_lengths, 0, T, out, bt.t1 - (bt.t_ship - bt.t0), bt.t1, f.n_readers);
}


// ---- a single-member gzip file (gzip, pigz, Python's gzip): inflated by speculative decoding --------------------------
// The header of a gzip member (RFC 1952 2.3) in the first n bytes of a file: where its deflate bytes begin.  false: not a
// header inflate would take (magic, CM != 8, reserved flag bits) or one that does not end within the n bytes.
bool gzip_head(const uint8_t* h, uint64_t n, uint64_t* deflate_off) {
    if (n < 10 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 0xE0) != 0) return false;
    const uint32_t flg = h[3];
    uint64_t o = 10;
    if (flg & 4) {                                                  // FEXTRA
        if (o + 2 > n) return false;
        o += 2 + (h[o] | (uint64_t)h[o + 1] << 8);
        if (o > n) return false;
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1) {                  // FNAME, FCOMMENT: zero-terminated
        if (!(flg & bit)) continue;
        const void* z = o < n ? memchr(h + o, 0, (size_t)(n - o)) : nullptr;
        if (!z) return false;
        o = (uint64_t)((const uint8_t*)z - h) + 1;
    }
    if (flg & 2) o += 2;                                            // FHCRC (not checked, as zlib's gzread does not)
    if (o > n) return false;
    *deflate_off = o;
    return true;
}

constexpr uint64_t kGzipHeadReach = 1u << 20;       // a header (name, comment, extra field) longer than this is the host reader's

struct GzipFile {
    uint64_t file_n = 0, text_n = 0;
    float ship_ms = 0;
    uint32_t n_readers = 0;
    rala_hip_gzip_timings tm = {};
};

// The whole file to the device, found / counted / chained / written / resolved there (inflate_kernels.hip), the text left in
// ctx->d_gzip_text with newlines behind it.  *valid = false: not a stream this can prove - a header the parse refuses, an
// invalid block on the chain, a final block that does not end at the trailer, a wrong ISIZE or CRC32.
int gzip_inflate(rala_hip_ctx* ctx, const char* path, uint32_t threads, GzipFile& g, bool* valid) {
    *valid = false;
    Fd file;
    file.fd = open(path, O_RDONLY);
    if (file.fd < 0) return ingest_fail(ctx, RALA_HIP_EINVAL, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(file.fd, &st) != 0 || !S_ISREG(st.st_mode)) return ingest_fail(ctx, RALA_HIP_ENOTAFILE, std::string("not a regular file: ") + path);
    const uint64_t file_n = g.file_n = (uint64_t)st.st_size;
    std::vector<uint8_t> head((size_t)std::min(file_n, kGzipHeadReach));
    uint8_t trailer[8];
    if (file_n < 18 || pread(file.fd, head.data(), head.size(), 0) != (ssize_t)head.size() ||
        pread(file.fd, trailer, 8, (off_t)(file_n - 8)) != 8) return RALA_HIP_OK;
    uint64_t deflate_off = 0;
    if (!gzip_head(head.data(), head.size(), &deflate_off) || deflate_off + 8 >= file_n) return RALA_HIP_OK;
    const uint64_t end = file_n - 8;
    const uint64_t chunk = (uint64_t)std::max<int64_t>(1024, ctx->gzip_chunk_bytes);
    const uint64_t n_chunks = (end - deflate_off + chunk - 1) / chunk;
    if (n_chunks >= 0x7FFFFFF0ull) return ingest_fail(ctx, RALA_HIP_ETOOLARGE, "file too large for 32-bit chunk ids");
    hipStream_t s = ctx->stream;
    const double t0 = now_ms();
    if (ctx->d_bgzf_comp.ensure(file_n + 64) != hipSuccess || ctx->d_gzip_starts.ensure(n_chunks) != hipSuccess ||
        ctx->d_gzip_spans.ensure(n_chunks * sizeof(GzipSpan)) != hipSuccess || ctx->d_bgzf_flag.ensure(1) != hipSuccess) {
        return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
    }
    const uint8_t* comp = ctx->d_bgzf_comp.p;
    INGEST_CHECK(hipMemsetAsync(ctx->d_bgzf_comp.p + file_n, 0, 64, s));
    INGEST_CHECK(hipMemsetAsync(ctx->d_bgzf_flag.p, 0, 4, s));
    if (ship_file(file.fd, 0, file_n, ctx->d_bgzf_comp.p, ctx->device, threads, nullptr, []() { return true; }, &g.n_readers)) {
        return ingest_fail(ctx, RALA_HIP_EDEVICE, std::string("reading / copying ") + path + " failed");
    }
    INGEST_CHECK(hipStreamSynchronize(s));
    const double t1 = now_ms();
    g.ship_ms = (float)(t1 - t0);
    // find, then count
    launch_gzip_find(comp, end, (file_n + 56) / 8, deflate_off, chunk, (uint32_t)n_chunks, ctx->debug_gzip_false_sync, ctx->d_gzip_starts.p, s);
    INGEST_CHECK(hipGetLastError());
    INGEST_CHECK(hipStreamSynchronize(s));
    const double t2 = now_ms();
    launch_gzip_count(comp, end, ctx->d_gzip_starts.p, (uint32_t)n_chunks, (GzipSpan*)ctx->d_gzip_spans.p, s);
    INGEST_CHECK(hipGetLastError());
    std::vector<uint64_t> starts(n_chunks);
    std::vector<GzipSpan> spans(n_chunks);
    INGEST_CHECK(hipMemcpyAsync(starts.data(), ctx->d_gzip_starts.p, n_chunks * 8, hipMemcpyDeviceToHost, s));
    INGEST_CHECK(hipMemcpyAsync(spans.data(), ctx->d_gzip_spans.p, n_chunks * sizeof(GzipSpan), hipMemcpyDeviceToHost, s));
    INGEST_CHECK(hipStreamSynchronize(s));
    const double t3 = now_ms();
    // the chain from chunk 0: the true chunks, their text offsets
    rala_hip_gzip_timings& tm = g.tm;
    tm.compressed_bytes = file_n;
    tm.chunks = n_chunks;
    for (uint64_t c = 1; c < n_chunks; ++c) tm.chunks_with_candidate += starts[c] != kGzipNoStart;
    std::vector<GzipJob> jobs;
    std::vector<uint64_t> text_off;
    uint64_t text_n = 0, end_bit = 0;
    for (uint64_t c = 0;;) {
        const GzipSpan& sp = spans[c];
        if (sp.status > 1 || (sp.status == 0 && (sp.next <= c || sp.next >= n_chunks))) return RALA_HIP_OK;
        GzipJob j;
        j.start_bit = starts[c];
        j.stop_bit = sp.status == 0 ? starts[sp.next] : kGzipNoStart;
        j.text_off = text_n;
        j.text_n = sp.text;
        j.first = jobs.empty() ? 1u : 0u;
        j.pad = 0;
        jobs.push_back(j);
        text_off.push_back(text_n);
        text_n += sp.text;
        tm.chunks_refuted += sp.refuted;
        tm.max_wave_text_bytes = std::max<uint64_t>(tm.max_wave_text_bytes, sp.text);
        if (sp.status == 1) { end_bit = sp.end_bit; break; }
        c = sp.next;
    }
    tm.chunks_confirmed = jobs.size() - 1;
    tm.text_bytes = text_n;
    tm.find_ms = (float)(t2 - t1);
    // the final block ends in the byte in front of the trailer; ISIZE
    if ((end_bit + 7) / 8 != end || (uint32_t)text_n != le32(trailer + 4)) return RALA_HIP_OK;
    const uint64_t n_seg = (text_n + gzip_segment_bytes() - 1) / gzip_segment_bytes();
    if (n_seg >= 0xFFFFFFF0ull) return ingest_fail(ctx, RALA_HIP_ETOOLARGE, "text too large for 32-bit segment ids");
    if (ctx->d_gzip_sym.ensure(text_n + 64) != hipSuccess || ctx->d_gzip_text.ensure(text_n + paf_chunk_bytes() + 8192) != hipSuccess ||
        ctx->d_gzip_jobs.ensure(jobs.size() * sizeof(GzipJob)) != hipSuccess || ctx->d_gzip_off.ensure(jobs.size()) != hipSuccess ||
        ctx->d_gzip_crc.ensure(n_seg + 1) != hipSuccess) {
        ctx->d_gzip_sym.release();
        ctx->d_gzip_text.release();
        return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the inflated text");
    }
    INGEST_CHECK(hipMemcpyAsync(ctx->d_gzip_jobs.p, jobs.data(), jobs.size() * sizeof(GzipJob), hipMemcpyHostToDevice, s));
    INGEST_CHECK(hipMemcpyAsync(ctx->d_gzip_off.p, text_off.data(), text_off.size() * 8, hipMemcpyHostToDevice, s));
    INGEST_CHECK(hipStreamSynchronize(s));
    const double t3b = now_ms();
    launch_gzip_write(comp, end, (const GzipJob*)ctx->d_gzip_jobs.p, (uint32_t)jobs.size(), ctx->d_gzip_sym.p, ctx->d_bgzf_flag.p, s);
    INGEST_CHECK(hipGetLastError());
    INGEST_CHECK(hipStreamSynchronize(s));
    const double t4 = now_ms();
    launch_gzip_resolve(ctx->d_gzip_sym.p, ctx->d_gzip_off.p, (uint32_t)jobs.size(), text_n, ctx->d_gzip_text.p, ctx->d_gzip_crc.p, ctx->d_bgzf_flag.p, s);
    INGEST_CHECK(hipGetLastError());
    // what lies behind the text reads as newlines (as for the plain file)
    INGEST_CHECK(hipMemsetAsync(ctx->d_gzip_text.p + text_n, '\n', paf_chunk_bytes() + 8192, s));
    std::vector<uint32_t> seg_crc(n_seg);
    uint32_t flag = 0;
    if (n_seg) INGEST_CHECK(hipMemcpyAsync(seg_crc.data(), ctx->d_gzip_crc.p, n_seg * 4, hipMemcpyDeviceToHost, s));
    INGEST_CHECK(hipMemcpyAsync(&flag, ctx->d_bgzf_flag.p, 4, hipMemcpyDeviceToHost, s));
    INGEST_CHECK(hipStreamSynchronize(s));
    const double t5 = now_ms();
    ctx->d_gzip_sym.release();
    ctx->d_bgzf_comp.release();
    tm.decode_ms = (float)((t3 - t2) + (t4 - t3b));        // the counting pass and the writing pass
    tm.resolve_ms = (float)(t5 - t4);
    if (flag || gzip_crc_of_segments(seg_crc.data(), text_n) != le32(trailer)) {
        ctx->d_gzip_text.release();
        return RALA_HIP_OK;
    }
    g.text_n = text_n;
    *valid = true;
    return RALA_HIP_OK;
}

// gzip's paf_tokenise_range: the lines that start in bytes [lo, hi) of the resident text
int gzip_tokenise_range(rala_hip_ctx* ctx, GzipFile& g, uint64_t lo, uint64_t hi, bool check_lengths, const PafTarget& T, PafRange* out) {
    *out = PafRange();
    hi = std::min(hi, g.text_n);
    lo = std::min(lo, hi);
    const uint64_t n = hi - lo;
    const uint64_t n_avail = std::min<uint64_t>(g.text_n - lo, n + paf_halo_bytes());
    const uint32_t chunk = paf_chunk_bytes();
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    if (n_chunks >= 0xFFFFFFF0ull) return ingest_fail(ctx, RALA_HIP_ETOOLARGE, "file too large for 32-bit chunk ids");
    if (!tokeniser_memory(ctx, n, n_chunks, 0, T)) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the overlap columns");
    const uint8_t* const text = ctx->d_gzip_text.p + lo;
    bool first_is_start = lo == 0;
    if (lo) {
        uint8_t before = 0;
        INGEST_CHECK(hipMemcpy(&before, text - 1, 1, hipMemcpyDeviceToHost));
        first_is_start = before == '\n';
    }
    out->file_bytes = g.file_n;
    const double t = now_ms();
    return tokenise_text(ctx, text, n, n_avail, first_is_start, check_lengths, 0, T, out, t, t, g.n_readers);
}

// ---- the sequence index: FASTA / FASTQ text -> names, lengths, offsets (sequence_kernels.hip) ----------------------
// One window of the text, in device memory at `text` (launch_sequence_count's layout): count, scan, the events and records
// written behind those of the windows before it, the names gathered behind theirs.  *flags: the kernels' verdict.
struct SequenceRun {
    bool fastq = false;
    uint64_t text_n = 0;
    uint64_t n_events = 0, n_stripped = 0, n_records = 0, name_bytes = 0;
    bool last_is_newline = true;        // the byte in front of the next window
};
int index_window(rala_hip_ctx* ctx, SequenceRun& R, const uint8_t* text, uint64_t lo, uint64_t n, uint64_t n_avail, uint32_t* flags) {
    hipStream_t s = ctx->stream;
    const uint64_t n_tiles = (n + sequence_tile_bytes() - 1) / sequence_tile_bytes();
    *flags = 0;
    if (!n_tiles) return RALA_HIP_OK;
    INGEST_CHECK(ctx->d_seq_tile[0].ensure(n_tiles + 2));
    INGEST_CHECK(ctx->d_seq_tile[1].ensure(n_tiles + 2));
    INGEST_CHECK(ctx->d_seq_flags.ensure(1));
    INGEST_CHECK(ctx->d_scan_ws.ensure(scan_workspace_bytes(n_tiles + 2)));
    launch_sequence_count(text, n, R.last_is_newline, R.fastq, ctx->d_seq_tile[0].p, ctx->d_seq_tile[1].p, s);
    launch_exclusive_scan(ctx->d_seq_tile[0].p, ctx->d_seq_tile[0].p, n_tiles, ctx->d_scan_ws.p, s);
    launch_exclusive_scan(ctx->d_seq_tile[1].p, ctx->d_seq_tile[1].p, n_tiles, ctx->d_scan_ws.p, s);
    uint32_t events = 0, stripped = 0;
    uint8_t last = 0;
    INGEST_CHECK(hipMemcpyAsync(&events, ctx->d_seq_tile[0].p + n_tiles, 4, hipMemcpyDeviceToHost, s));
    INGEST_CHECK(hipMemcpyAsync(&stripped, ctx->d_seq_tile[1].p + n_tiles, 4, hipMemcpyDeviceToHost, s));
    INGEST_CHECK(hipMemcpyAsync(&last, text + n - 1, 1, hipMemcpyDeviceToHost, s));
    INGEST_CHECK(hipStreamSynchronize(s));
    INGEST_CHECK(hipGetLastError());
    // (a FASTQ record is four events; one whose lines are spread over two windows is counted where its header lies)
    const uint64_t ev_after = R.n_events + events;
    const uint64_t rec_before = R.n_records, rec_after = R.fastq ? (ev_after + 3) / 4 : ev_after;
    if (ctx->d_seq_event[0].grow(R.n_events, ev_after + 1) != hipSuccess || ctx->d_seq_event[1].grow(R.n_events, ev_after + 1) != hipSuccess ||
        ctx->d_seq_name_pos.grow(rec_before, rec_after + 1) != hipSuccess || ctx->d_seq_name_len.grow(rec_before, rec_after + 1) != hipSuccess ||
        ctx->d_seq_data_off.grow(rec_before, rec_after + 1) != hipSuccess || ctx->d_seq_data_stripped.grow(rec_before, rec_after + 1) != hipSuccess ||
        ctx->d_seq_name_off.grow(rec_before, rec_after + 1) != hipSuccess) {
        return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the sequence index");
    }
    INGEST_CHECK(hipMemsetAsync(ctx->d_seq_flags.p, 0, 4, s));
    SequenceWindow W;
    W.text = text; W.n = n; W.n_avail = n_avail; W.text_off = lo; W.text_n = R.text_n;
    W.first_is_start = R.last_is_newline ? 1u : 0u;
    W.tile_event0 = ctx->d_seq_tile[0].p; W.tile_stripped0 = ctx->d_seq_tile[1].p;
    W.event0 = R.n_events; W.stripped0 = R.n_stripped;
    SequenceColumns C;
    C.event_pos = ctx->d_seq_event[0].p; C.event_stripped = ctx->d_seq_event[1].p;
    C.name_pos = ctx->d_seq_name_pos.p; C.name_len = ctx->d_seq_name_len.p;
    C.data_off = ctx->d_seq_data_off.p; C.data_stripped = ctx->d_seq_data_stripped.p;
    launch_sequence_records(W, R.fastq, C, ctx->d_seq_flags.p, s);
    INGEST_CHECK(hipGetLastError());
    // the headers of this window: FASTA - every event; FASTQ - the events 4r
    const uint64_t hdr_before = R.fastq ? (R.n_events + 3) / 4 : R.n_events;
    const uint64_t n_hdr = rec_after - hdr_before;
    uint32_t bytes = 0;
    if (n_hdr) {
        INGEST_CHECK(ctx->d_seq_name_at.ensure(n_hdr + 2));
        INGEST_CHECK(ctx->d_scan_ws.ensure(scan_workspace_bytes(n_hdr + 2)));
        launch_exclusive_scan(ctx->d_seq_name_len.p + hdr_before, ctx->d_seq_name_at.p, n_hdr, ctx->d_scan_ws.p, s);
        INGEST_CHECK(hipMemcpyAsync(&bytes, ctx->d_seq_name_at.p + n_hdr, 4, hipMemcpyDeviceToHost, s));
    }
    INGEST_CHECK(hipMemcpyAsync(flags, ctx->d_seq_flags.p, 4, hipMemcpyDeviceToHost, s));
    INGEST_CHECK(hipStreamSynchronize(s));
    if (*flags) return RALA_HIP_OK;
    if (n_hdr) {
        if (ctx->d_seq_arena.grow(R.name_bytes, R.name_bytes + bytes + 1) != hipSuccess) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the names");
        launch_sequence_names(text, lo, ctx->d_seq_name_pos.p + hdr_before, ctx->d_seq_name_len.p + hdr_before, ctx->d_seq_name_at.p, n_hdr,
                              R.name_bytes, ctx->d_seq_arena.p, ctx->d_seq_name_off.p + hdr_before, s);
        INGEST_CHECK(hipGetLastError());
        INGEST_CHECK(hipStreamSynchronize(s));
    }
    R.n_events = ev_after;
    R.n_stripped += stripped;
    R.n_records = rec_after;
    R.name_bytes += bytes;
    R.last_is_newline = last == '\n';
    return RALA_HIP_OK;
}

// ---- a single-member gzip read file, inflated WINDOW by window (the driver of gzip_inflate's kernels for a text that does
// not fit): find, count and the chain run over the whole compressed file, which stays resident - the only buffer whose size
// depends on the file's; write, windows and resolve then run per window, a run of consecutive true chunks whose text fits
// it.  The symbols of a window lie behind a CARRY of gzip_ring_symbols(): the last 32 768 bytes in front of it (0x8000 where
// the file's text has not begun), so the markers of its first chunks point into bytes, and every text offset the kernels see
// counts from the carry's first symbol.
struct GzipWalk {
    std::vector<GzipJob> chain;             // the true chunks, text offsets from the text's start
    uint64_t file_n = 0, end = 0, text_n = 0;
    uint32_t crc = 0;                       // the trailer's
    uint64_t window = 0;                    // text bytes a window holds at most (at least the largest chunk's)
    size_t next_job = 0;
    std::vector<uint32_t> reg;              // the windows' CRC registers and lengths
    std::vector<uint64_t> len;
    float ship_ms = 0;
    uint32_t n_readers = 0;
    rala_hip_gzip_timings tm = {};
};

// The file to the device and (chain == null) its chain built there, or the chain of an earlier walk taken over; the buffers
// of a window made: `front` bytes of room in front of the window's text in ctx->d_gzip_text and `behind` bytes behind it.
// want_window 0: what a quarter of the free memory holds at three bytes per text byte.  *valid = false: not a stream this can prove.
int gzip_walk_open(rala_hip_ctx* ctx, int fd, const char* path, uint32_t threads, uint64_t want_window, uint64_t front, uint64_t behind,
                   const std::vector<GzipJob>* chain, GzipWalk& g, bool* valid) {
    *valid = false;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return ingest_fail(ctx, RALA_HIP_ENOTAFILE, std::string("not a regular file: ") + path);
    const uint64_t file_n = g.file_n = (uint64_t)st.st_size;
    std::vector<uint8_t> head((size_t)std::min(file_n, kGzipHeadReach));
    uint8_t trailer[8];
    if (file_n < 18 || pread(fd, head.data(), head.size(), 0) != (ssize_t)head.size() || pread(fd, trailer, 8, (off_t)(file_n - 8)) != 8) return RALA_HIP_OK;
    uint64_t deflate_off = 0;
    if (!gzip_head(head.data(), head.size(), &deflate_off) || deflate_off + 8 >= file_n) return RALA_HIP_OK;
    const uint64_t end = g.end = file_n - 8;
    g.crc = le32(trailer);
    hipStream_t s = ctx->stream;
    const double t0 = now_ms();
    if (ctx->d_bgzf_comp.ensure(file_n + 64) != hipSuccess || ctx->d_bgzf_flag.ensure(1) != hipSuccess) {
        return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
    }
    const uint8_t* comp = ctx->d_bgzf_comp.p;
    INGEST_CHECK(hipMemsetAsync(ctx->d_bgzf_comp.p + file_n, 0, 64, s));
    INGEST_CHECK(hipMemsetAsync(ctx->d_bgzf_flag.p, 0, 4, s));
    if (ship_file(fd, 0, file_n, ctx->d_bgzf_comp.p, ctx->device, threads, nullptr, []() { return true; }, &g.n_readers)) {
        return ingest_fail(ctx, RALA_HIP_EDEVICE, std::string("reading / copying ") + path + " failed");
    }
    INGEST_CHECK(hipStreamSynchronize(s));
    const double t1 = now_ms();
    g.ship_ms = (float)(t1 - t0);
    rala_hip_gzip_timings& tm = g.tm;
    tm.compressed_bytes = file_n;
    if (chain) {
        g.chain = *chain;
        for (const GzipJob& j : g.chain) {
            g.text_n += j.text_n;
            tm.max_wave_text_bytes = std::max<uint64_t>(tm.max_wave_text_bytes, j.text_n);
        }
        tm.chunks_confirmed = g.chain.size() - 1;
        if (g.chain.empty() || (uint32_t)g.text_n != le32(trailer + 4)) return RALA_HIP_OK;
    } else {
        const uint64_t chunk = (uint64_t)std::max<int64_t>(1024, ctx->gzip_chunk_bytes);
        const uint64_t n_chunks = (end - deflate_off + chunk - 1) / chunk;
        if (n_chunks >= 0x7FFFFFF0ull) return ingest_fail(ctx, RALA_HIP_ETOOLARGE, "file too large for 32-bit chunk ids");
        if (ctx->d_gzip_starts.ensure(n_chunks) != hipSuccess || ctx->d_gzip_spans.ensure(n_chunks * sizeof(GzipSpan)) != hipSuccess) {
            return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
        }
        launch_gzip_find(comp, end, (file_n + 56) / 8, deflate_off, chunk, (uint32_t)n_chunks, ctx->debug_gzip_false_sync, ctx->d_gzip_starts.p, s);
        INGEST_CHECK(hipGetLastError());
        INGEST_CHECK(hipStreamSynchronize(s));
        const double t2 = now_ms();
        launch_gzip_count(comp, end, ctx->d_gzip_starts.p, (uint32_t)n_chunks, (GzipSpan*)ctx->d_gzip_spans.p, s);
        INGEST_CHECK(hipGetLastError());
        std::vector<uint64_t> starts(n_chunks);
        std::vector<GzipSpan> spans(n_chunks);
        INGEST_CHECK(hipMemcpyAsync(starts.data(), ctx->d_gzip_starts.p, n_chunks * 8, hipMemcpyDeviceToHost, s));
        INGEST_CHECK(hipMemcpyAsync(spans.data(), ctx->d_gzip_spans.p, n_chunks * sizeof(GzipSpan), hipMemcpyDeviceToHost, s));
        INGEST_CHECK(hipStreamSynchronize(s));
        const double t3 = now_ms();
        ctx->d_gzip_starts.release();
        ctx->d_gzip_spans.release();
        tm.chunks = n_chunks;
        tm.find_ms = (float)(t2 - t1);
        tm.decode_ms = (float)(t3 - t2);
        for (uint64_t c = 1; c < n_chunks; ++c) tm.chunks_with_candidate += starts[c] != kGzipNoStart;
        // the chain from chunk 0: the true chunks, their text offsets
        uint64_t text_n = 0, end_bit = 0;
        for (uint64_t c = 0;;) {
            const GzipSpan& sp = spans[c];
            if (sp.status > 1 || (sp.status == 0 && (sp.next <= c || sp.next >= n_chunks))) return RALA_HIP_OK;
            GzipJob j;
            j.start_bit = starts[c];
            j.stop_bit = sp.status == 0 ? starts[sp.next] : kGzipNoStart;
            j.text_off = text_n;
            j.text_n = sp.text;
            j.first = g.chain.empty() ? 1u : 0u;
            j.pad = 0;
            g.chain.push_back(j);
            text_n += sp.text;
            tm.chunks_refuted += sp.refuted;
            tm.max_wave_text_bytes = std::max<uint64_t>(tm.max_wave_text_bytes, sp.text);
            if (sp.status == 1) { end_bit = sp.end_bit; break; }
            c = sp.next;
        }
        tm.chunks_confirmed = g.chain.size() - 1;
        // the final block ends in the byte in front of the trailer; ISIZE
        if ((end_bit + 7) / 8 != end || (uint32_t)text_n != le32(trailer + 4)) return RALA_HIP_OK;
        g.text_n = text_n;
    }
    tm.text_bytes = g.text_n;
    // the window: symbols (2 bytes) and text (1 byte) of it inside the quarter of what is free now
    uint64_t window = want_window;
    if (window == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        window = std::max<uint64_t>(64ull << 20, free_b / 12);
    }
    window = std::max<uint64_t>(std::min<uint64_t>(window, 1ull << 31), tm.max_wave_text_bytes);
    if (window > (1ull << 31)) return ingest_fail(ctx, RALA_HIP_ENOMEM, "a chunk of the gzip file gives more text than a window holds");
    window = std::min(window, std::max<uint64_t>(g.text_n, 1));
    g.window = window;
    const uint64_t ring = gzip_ring_symbols();
    if (ctx->d_gzip_sym.ensure(ring + window + 64) != hipSuccess || ctx->d_gzip_text.ensure(front + window + behind) != hipSuccess ||
        ctx->d_gzip_crc.ensure(window / gzip_segment_bytes() + 2) != hipSuccess || ctx->d_gzip_carry.ensure(ring) != hipSuccess ||
        ctx->d_gzip_hold.ensure(front + 16) != hipSuccess) {
        ctx->d_gzip_sym.release();
        ctx->d_gzip_text.release();
        return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for a window of the inflated text");
    }
    // nothing lies in front of the first window: a marker that points there is no byte
    INGEST_CHECK(hipMemsetD16Async((hipDeviceptr_t)ctx->d_gzip_sym.p, (unsigned short)0x8000u, ring, s));
    *valid = true;
    return RALA_HIP_OK;
}

// The next window's text [*lo, *lo + *n) to `text` (16-byte aligned, in ctx->d_gzip_text).  *flag != 0: the inflater refused.
int gzip_walk_next(rala_hip_ctx* ctx, GzipWalk& g, uint8_t* text, uint64_t* lo, uint64_t* n, uint32_t* flag) {
    hipStream_t s = ctx->stream;
    const uint64_t ring = gzip_ring_symbols();
    const size_t j0 = g.next_job;
    size_t j1 = j0;
    uint64_t n_w = 0;
    while (j1 < g.chain.size() && (j1 == j0 || n_w + g.chain[j1].text_n <= g.window)) n_w += g.chain[j1++].text_n;
    const uint64_t a = g.chain[j0].text_off;
    std::vector<GzipJob> jobs(g.chain.begin() + j0, g.chain.begin() + j1);
    std::vector<uint64_t> text_off(jobs.size());
    for (size_t j = 0; j < jobs.size(); ++j) text_off[j] = jobs[j].text_off = ring + (jobs[j].text_off - a);
    if (n_w > g.window) return ingest_fail(ctx, RALA_HIP_EDEVICE, "a chunk larger than the window");
    *lo = a;
    *n = n_w;
    *flag = 0;
    g.next_job = j1;
    if (ctx->d_gzip_jobs.ensure(jobs.size() * sizeof(GzipJob)) != hipSuccess || ctx->d_gzip_off.ensure(jobs.size()) != hipSuccess) {
        return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for a window's chunks");
    }
    const double t0 = now_ms();
    INGEST_CHECK(hipMemcpyAsync(ctx->d_gzip_jobs.p, jobs.data(), jobs.size() * sizeof(GzipJob), hipMemcpyHostToDevice, s));
    INGEST_CHECK(hipMemcpyAsync(ctx->d_gzip_off.p, text_off.data(), text_off.size() * 8, hipMemcpyHostToDevice, s));
    launch_gzip_write(ctx->d_bgzf_comp.p, g.end, (const GzipJob*)ctx->d_gzip_jobs.p, (uint32_t)jobs.size(), ctx->d_gzip_sym.p, ctx->d_bgzf_flag.p, s);
    INGEST_CHECK(hipGetLastError());
    INGEST_CHECK(hipStreamSynchronize(s));
    const double t1 = now_ms();
    const uint64_t n_seg = (n_w + gzip_segment_bytes() - 1) / gzip_segment_bytes();
    launch_gzip_resolve(ctx->d_gzip_sym.p, ctx->d_gzip_off.p, (uint32_t)jobs.size(), n_w, text, ctx->d_gzip_crc.p, ctx->d_bgzf_flag.p, s, ring);
    INGEST_CHECK(hipGetLastError());
    std::vector<uint32_t> seg_crc(n_seg);
    if (n_seg) INGEST_CHECK(hipMemcpyAsync(seg_crc.data(), ctx->d_gzip_crc.p, n_seg * 4, hipMemcpyDeviceToHost, s));
    INGEST_CHECK(hipMemcpyAsync(flag, ctx->d_bgzf_flag.p, 4, hipMemcpyDeviceToHost, s));
    if (j1 < g.chain.size()) launch_gzip_carry(ctx->d_gzip_sym.p, text, n_w, ctx->d_gzip_carry.p, s);
    INGEST_CHECK(hipGetLastError());
    INGEST_CHECK(hipStreamSynchronize(s));
    g.tm.decode_ms += (float)(t1 - t0);
    g.tm.resolve_ms += (float)(now_ms() - t1);
    g.reg.push_back(gzip_crc_register(seg_crc.data(), n_w));
    g.len.push_back(n_w);
    return RALA_HIP_OK;
}

// behind the last window: is the text the trailer's?
bool gzip_walk_proven(const GzipWalk& g) {
    return g.next_job == g.chain.size() && gzip_crc_chain(g.reg.data(), g.len.data(), g.reg.size()) == g.crc;
}

// ---- the text of a read file window by window: a plain file's bytes, a BGZF file's members, a gzip member's chunks ------
// Both passes walk it: rala_hip_index_sequences and rala_hip_slice_sequences.  A window is the n bytes at text position lo
// that are this step's, and behind them what of the next sequence_halo_bytes() the text still has (n_avail); zeros behind
// those up to the next multiple of the tile + the halo + 64.  The gzip source inflates whole chunks: it holds the tail of
// every inflated window back and puts it in front of the next one.
struct TextWindow {
    const uint8_t* text = nullptr;
    uint64_t lo = 0, n = 0, n_avail = 0;
    double t_kernels = 0;                   // from here on the device works on the window (what was before: the ship)
};
struct TextSource {
    int kind = 0;                           // 0 plain, 1 BGZF, 2 gzip
    int fd = -1;
    std::string path;
    uint32_t threads = 1;
    uint64_t window = 0, file_n = 0, text_n = 0;
    std::unique_ptr<BgzfFile> bg;
    std::unique_ptr<GzipWalk> gz;
    uint64_t lo = 0, hold = 0, front = 0;
    double ship_ms = 0;
    uint32_t flag = 0;                      // 8: an inflater refused
    uint64_t windows = 0, max_window = 0;
};

uint64_t sequence_window_bytes(rala_hip_ctx* ctx) {
    uint64_t window = (uint64_t)ctx->debug_sequence_window;
    if (window == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        window = std::max<uint64_t>(256ull << 20, free_b / 4);
    }
    return std::min<uint64_t>(window, 1ull << 31);
}

// *valid = false: a gzip file this does not take (not BGZF and gzip_ok false, or one the inflaters cannot prove)
int source_open(rala_hip_ctx* ctx, TextSource& S, bool gzip_ok, const std::vector<GzipJob>* chain, bool* valid) {
    *valid = true;
    S.text_n = S.file_n;
    S.window = sequence_window_bytes(ctx);
    uint8_t head[18] = {0};
    const ssize_t got = pread(S.fd, head, sizeof(head), 0);
    if (!(got >= 2 && head[0] == 0x1f && head[1] == 0x8b)) return RALA_HIP_OK;
    *valid = bgzf_head(head, (uint64_t)got);
    if (*valid) {
        S.kind = 1;
        S.bg.reset(new BgzfFile);
        const int rc = bgzf_open(ctx, S.path.c_str(), S.threads, S.window, *S.bg, valid);
        if (rc != RALA_HIP_OK) return rc;
        S.text_n = S.bg->text_n;
        S.ship_ms = S.bg->ship_ms;
    } else if (gzip_ok) {
        S.kind = 2;
        S.gz.reset(new GzipWalk);
        const uint64_t tile = sequence_tile_bytes(), halo = sequence_halo_bytes();
        S.front = (halo + 15) / 16 * 16;
        const int rc = gzip_walk_open(ctx, S.fd, S.path.c_str(), S.threads, (uint64_t)ctx->debug_sequence_window, S.front, tile + halo + 64 + 16, chain,
                                      *S.gz, valid);
        if (rc != RALA_HIP_OK) return rc;
        S.text_n = S.gz->text_n;
        S.ship_ms = S.gz->ship_ms;
    }
    return RALA_HIP_OK;
}

int source_next(rala_hip_ctx* ctx, TextSource& S, TextWindow* w) {
    hipStream_t s = ctx->stream;
    const uint64_t tile = sequence_tile_bytes(), halo = sequence_halo_bytes();
    const double t0 = now_ms();
    w->lo = S.lo;
    if (S.kind == 2) {
        uint8_t* const at = ctx->d_gzip_text.p + S.front;
        uint64_t a = 0, n_w = 0;
        const int rc = gzip_walk_next(ctx, *S.gz, at, &a, &n_w, &S.flag);
        if (rc != RALA_HIP_OK || S.flag) return rc;
        if (a != S.lo + S.hold) return ingest_fail(ctx, RALA_HIP_EDEVICE, "the gzip windows do not follow each other");
        uint8_t* text = at - S.hold;
        w->n_avail = S.hold + n_w;
        const bool last = a + n_w == S.text_n;
        w->n = last ? w->n_avail : w->n_avail > halo ? w->n_avail - halo : 0;
        const uint64_t cap = (w->n + tile - 1) / tile * tile + halo + 64;
        // What is held back is the halo, a multiple of 16, unless the windows so far were no longer than it: then all of
        // them is held back, any number of bytes, and the text in front of `at` does not begin at a multiple of 16, where
        // the index's and the slicer's kernels load it 16 bytes at a time.  Such a window goes to a buffer of its own.
        if (S.hold % 16) {
            if (ctx->d_paf_text.ensure(cap) != hipSuccess) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for a window of the inflated text");
            INGEST_CHECK(hipMemcpyAsync(ctx->d_paf_text.p, text, w->n_avail, hipMemcpyDeviceToDevice, s));
            text = ctx->d_paf_text.p;
        }
        INGEST_CHECK(hipMemsetAsync(text + w->n_avail, 0, cap - w->n_avail, s));
        INGEST_CHECK(hipStreamSynchronize(s));
        w->text = text;
        w->t_kernels = t0;
    } else {
        w->n = std::min(S.window, S.text_n - S.lo);
        w->n_avail = std::min<uint64_t>(S.text_n - S.lo, w->n + halo);
        const uint64_t cap = (w->n + tile - 1) / tile * tile + halo + 64;
        // what lies behind the text reads as zeros: a carriage return in the text's last byte is a base, as on the host
        if (S.kind == 1) {
            BgzfText bt;
            const int rc = bgzf_text_range(ctx, *S.bg, S.lo, w->n_avail, cap, 0, S.threads, []() { return true; }, "device memory", &bt);
            if (rc != RALA_HIP_OK) return rc;
            if (bt.flag) { S.flag = 8; return RALA_HIP_OK; }
            w->text = bt.text;
            w->t_kernels = bt.t1;
            S.ship_ms += bt.t_ship - bt.t0;
        } else {
            if (ctx->d_paf_text.ensure(cap) != hipSuccess) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the file's text");
            if (hipMemsetAsync(ctx->d_paf_text.p + w->n_avail, 0, cap - w->n_avail, s) != hipSuccess ||
                ship_file(S.fd, S.lo, w->n_avail, ctx->d_paf_text.p, ctx->device, S.threads, nullptr, []() { return true; }, nullptr) ||
                hipStreamSynchronize(s) != hipSuccess) {
                return ingest_fail(ctx, RALA_HIP_EDEVICE, "reading / copying " + S.path + " failed");
            }
            w->text = ctx->d_paf_text.p;
            w->t_kernels = now_ms();
            S.ship_ms += w->t_kernels - t0;
        }
    }
    ++S.windows;
    S.max_window = std::max(S.max_window, w->n_avail);
    return RALA_HIP_OK;
}

// the window is done with: on to the next one (gzip: what was held back goes in front of it)
int source_advance(rala_hip_ctx* ctx, TextSource& S, const TextWindow& w) {
    S.lo = w.lo + w.n;
    if (S.kind != 2) return RALA_HIP_OK;
    S.hold = w.n_avail - w.n;
    if (S.hold && S.lo < S.text_n) {
        hipStream_t s = ctx->stream;
        INGEST_CHECK(hipMemcpyAsync(ctx->d_gzip_hold.p, w.text + w.n, S.hold, hipMemcpyDeviceToDevice, s));
        INGEST_CHECK(hipMemcpyAsync(ctx->d_gzip_text.p + S.front - S.hold, ctx->d_gzip_hold.p, S.hold, hipMemcpyDeviceToDevice, s));
        INGEST_CHECK(hipStreamSynchronize(s));
    }
    return RALA_HIP_OK;
}

void source_close(rala_hip_ctx* ctx) {
    ctx->d_paf_text.release();                  // (a window of the file: not kept)
    ctx->d_bgzf_comp.release();
    ctx->d_gzip_sym.release();
    ctx->d_gzip_text.release();
}

void trace_gzip_walk(const GzipWalk& g) {
    const rala_hip_gzip_timings& t = g.tm;
    fprintf(stderr, "[trace] device inflate: one gzip member in %lu windows of at most %.3f GB of text, %.3f GB compressed shipped in %.1f ms, %lu "
            "chunks (%lu with a candidate, %lu confirmed, %lu refuted), %.3f GB of text (at most %.3f GB by one wave): find %.2f ms, decode %.2f ms, "
            "resolve %.2f ms\n", (unsigned long)g.reg.size(), g.window / 1e9, t.compressed_bytes / 1e9, g.ship_ms, (unsigned long)t.chunks,
            (unsigned long)t.chunks_with_candidate, (unsigned long)t.chunks_confirmed, (unsigned long)t.chunks_refuted, t.text_bytes / 1e9,
            t.max_wave_text_bytes / 1e9, t.find_ms, t.decode_ms, t.resolve_ms);
}

}  // namespace

extern "C" {

int rala_hip_set_name_table(rala_hip_ctx* ctx, const void* buckets, uint64_t n_buckets, const char* arena, uint64_t arena_bytes) {
    if (!ctx || !buckets || n_buckets == 0 || (n_buckets & (n_buckets - 1)) != 0 || (!arena && arena_bytes)) return RALA_HIP_EINVAL;
    INGEST_CHECK(hipSetDevice(ctx->device));
    INGEST_CHECK(ctx->d_name_buckets.ensure(n_buckets * sizeof(NameBucket)));
    INGEST_CHECK(ctx->d_name_arena.ensure(arena_bytes + 16));
    INGEST_CHECK(hipMemcpy(ctx->d_name_buckets.p, buckets, n_buckets * sizeof(NameBucket), hipMemcpyHostToDevice));
    if (arena_bytes) INGEST_CHECK(hipMemcpy(ctx->d_name_arena.p, arena, arena_bytes, hipMemcpyHostToDevice));
    ctx->n_name_buckets = n_buckets;
    return RALA_HIP_OK;
}

static int set_overlaps_from_text(rala_hip_ctx* ctx, const char* path, bool mhap, int check_lengths, uint32_t threads,
                                  int64_t* length_error_read, int* irregular);

int rala_hip_set_overlaps_from_paf(rala_hip_ctx* ctx, const char* path, int check_lengths, uint32_t threads,
                                   int64_t* length_error_read, int* irregular) {
    return set_overlaps_from_text(ctx, path, false, check_lengths, threads, length_error_read, irregular);
}

int rala_hip_set_overlaps_from_mhap(rala_hip_ctx* ctx, const char* path, int check_lengths, uint32_t threads,
                                    int64_t* length_error_read, int* irregular) {
    return set_overlaps_from_text(ctx, path, true, check_lengths, threads, length_error_read, irregular);
}

static int set_overlaps_from_text(rala_hip_ctx* ctx, const char* path, bool mhap, int check_lengths, uint32_t threads,
                                  int64_t* length_error_read, int* irregular) {
    if (!ctx || !path || !length_error_read || !irregular) return RALA_HIP_EINVAL;
    *length_error_read = -1;
    *irregular = 0;
    // (the columns a successful call before this one left are about to be written over - whatever happens
    // here, the context has no overlaps until this call has set them)
    ctx->inputs_set = false;
    ctx->n_ovl = 0;
    ctx->ovl = OvlSoA();
    ctx->initialized = ctx->constructed = false;
    PafTarget T;
    for (int k = 0; k < 7; ++k) T.col[k] = &ctx->d_paf_col[k];
    T.strand = &ctx->d_paf_strand;
    T.mhap = mhap;
    PafRange R;
    // The file's text goes through device memory in WINDOWS (round 5; before, all of it had to fit at once): at most a
    // quarter of what is free (option ingest_window_bytes; the reference streams the file in chunks of 1 GiB,
    // graph.cpp:24, 329-365 - its run carry-over is not needed here, rows are tokenised independently of each other and
    // a window takes the lines that START in it).  One window - the usual case - tokenises straight into the columns.
    uint64_t window = (uint64_t)ctx->ingest_window_bytes;
    if (window == 0 && getenv("RALA_INGEST_WINDOW")) window = (uint64_t)atoll(getenv("RALA_INGEST_WINDOW"));      // (tests)
    if (window == 0) {
        size_t free_b = 0, total_b = 0;
        INGEST_CHECK(hipSetDevice(ctx->device));
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        window = std::max<uint64_t>(256ull << 20, free_b / 4);
    }
    struct stat st_;
    uint64_t file_n = stat(path, &st_) == 0 && S_ISREG(st_.st_mode) ? (uint64_t)st_.st_size : 0;
    // A gzip file: BGZF is inflated on the device (the windows then lie over its text), anything else is the host reader's -
    // known from the first 18 bytes, before anything is shipped
    ctx->inflate_tm = rala_hip_inflate_timings();
    ctx->gzip_tm = rala_hip_gzip_timings();
    std::unique_ptr<BgzfFile> bg;
    std::unique_ptr<GzipFile> gz;
    if (file_n >= 2) {
        uint8_t head[18] = {0};
        ssize_t got = -1;
        {
            Fd probe;
            probe.fd = open(path, O_RDONLY);
            if (probe.fd >= 0) got = pread(probe.fd, head, sizeof(head), 0);
        }
        if (got >= 2 && head[0] == 0x1f && head[1] == 0x8b) {
            bool valid = bgzf_head(head, (uint64_t)got);
            if (!valid && ctx->gzip_on_device) {
                // (option gzip_on_device) any other gzip file: one member, inflated by speculative decoding - the whole text
                // is resident afterwards, the windows lie over it
                if (ctx->n_reads == 0) return ingest_fail(ctx, RALA_HIP_EINVAL, "no reads set");
                if (ctx->n_name_buckets == 0 && !mhap) return ingest_fail(ctx, RALA_HIP_EINVAL, "no name table set (rala_hip_set_name_table)");
                INGEST_CHECK(hipSetDevice(ctx->device));
                gz.reset(new GzipFile);
                const int rc = gzip_inflate(ctx, path, threads, *gz, &valid);
                ctx->gzip_tm = gz->tm;
                if (rc != RALA_HIP_OK || !valid) {
                    ctx->d_bgzf_comp.release();
                    ctx->d_gzip_sym.release();
                    ctx->d_gzip_text.release();
                    if (rc != RALA_HIP_OK) return rc;
                    *irregular = 8;
                    return RALA_HIP_OK;
                }
                file_n = gz->text_n;
            } else if (valid) {
                if (ctx->n_reads == 0) return ingest_fail(ctx, RALA_HIP_EINVAL, "no reads set");
                if (ctx->n_name_buckets == 0 && !mhap) return ingest_fail(ctx, RALA_HIP_EINVAL, "no name table set (rala_hip_set_name_table)");
                INGEST_CHECK(hipSetDevice(ctx->device));
                bg.reset(new BgzfFile);
                const int rc = bgzf_open(ctx, path, threads, window, *bg, &valid);
                if (rc != RALA_HIP_OK) return rc;
            }
            if (!valid) {
                *irregular = 8;
                return RALA_HIP_OK;
            }
            if (bg) file_n = bg->text_n;
        }
    }
    auto tokenise_range = [&](uint64_t lo, uint64_t hi, const PafTarget& to, PafRange* part) {
        return gz ? gzip_tokenise_range(ctx, *gz, lo, hi, check_lengths != 0, to, part) :
               bg ? bgzf_tokenise_range(ctx, *bg, lo, hi, check_lengths != 0, threads, to, part)
                  : paf_tokenise_range(ctx, path, lo, hi, check_lengths != 0, threads, 0, to, part);
    };
    if (file_n <= window) {
        const int rc = tokenise_range(0, ~0ull, T, &R);
        if (rc != RALA_HIP_OK) return rc;
    } else {
        PafTarget W;
        for (int k = 0; k < 7; ++k) W.col[k] = &ctx->d_paf_win[k];
        W.strand = &ctx->d_paf_win_strand;
        W.mhap = mhap;
        uint64_t rows = 0;
        float ship = 0, tok = 0;
        for (uint64_t lo = 0; lo < file_n; lo += window) {
            PafRange part;
            const int rc = tokenise_range(lo, lo + window, W, &part);
            if (rc != RALA_HIP_OK) return rc;
            ship += ctx->ingest_tm.ship_ms; tok += ctx->ingest_tm.tokenize_ms;
            R.flags |= part.flags;
            if (part.flags) break;
            if (part.first_bad != ~0ull) {          // (windows come in file order: the first one with an offender holds the first offender)
                R.first_bad = (((part.first_bad >> 32) + rows) << 32) | (part.first_bad & 0xFFFFFFFFull);
                break;
            }
            if (rows + part.n_lines >= 0xFFFFFFF0ull / 2) return ingest_fail(ctx, RALA_HIP_ETOOLARGE, "too many overlaps for 32-bit bound offsets");
            for (int k = 0; k < 7; ++k) {
                if (ctx->d_paf_col[k].grow(rows, rows + part.n_lines + 1) != hipSuccess) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the overlap columns");
                if (part.n_lines) INGEST_CHECK(hipMemcpy(ctx->d_paf_col[k].p + rows, ctx->d_paf_win[k].p, part.n_lines * 4, hipMemcpyDeviceToDevice));
            }
            if (ctx->d_paf_strand.grow(rows, rows + part.n_lines + 1) != hipSuccess) return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the overlap columns");
            if (part.n_lines) INGEST_CHECK(hipMemcpy(ctx->d_paf_strand.p + rows, ctx->d_paf_win_strand.p, part.n_lines, hipMemcpyDeviceToDevice));
            rows += part.n_lines;
        }
        for (int k = 0; k < 7; ++k) ctx->d_paf_win[k].release();
        ctx->d_paf_win_strand.release();
        R.n_lines = rows;
        ctx->ingest_tm.ship_ms = ship; ctx->ingest_tm.tokenize_ms = tok;
        ctx->ingest_tm.bytes = file_n; ctx->ingest_tm.lines = rows;
    }
    if (bg) {
        ctx->d_bgzf_comp.release();
        ctx->ingest_tm.ship_ms += bg->ship_ms;
        ctx->inflate_tm.inflate_ms = bg->inflate_ms;
        ctx->inflate_tm.compressed_bytes = bg->shipped;
        ctx->inflate_tm.members = bg->jobs.size();
        if (getenv("RALA_HIP_TRACE")) {
            fprintf(stderr, "[trace] device inflate: %lu BGZF members, %.3f GB compressed shipped (index and ship %.1f ms), %.3f GB of text "
                    "inflated in %.2f ms\n", (unsigned long)bg->jobs.size(), bg->shipped / 1e9, bg->ship_ms, bg->text_n / 1e9, bg->inflate_ms);
        }
    }
    if (gz) {
        ctx->d_gzip_text.release();
        ctx->ingest_tm.ship_ms += gz->ship_ms;
        if (getenv("RALA_HIP_TRACE")) {
            const rala_hip_gzip_timings& g = ctx->gzip_tm;
            fprintf(stderr, "[trace] device inflate: one gzip member, %.3f GB compressed shipped in %.1f ms, %lu chunks (%lu with a candidate, %lu "
                    "confirmed, %lu refuted), %.3f GB of text (at most %.3f GB by one wave): find %.2f ms, decode %.2f ms, resolve %.2f ms\n",
                    g.compressed_bytes / 1e9, gz->ship_ms, (unsigned long)g.chunks, (unsigned long)g.chunks_with_candidate,
                    (unsigned long)g.chunks_confirmed, (unsigned long)g.chunks_refuted, g.text_bytes / 1e9, g.max_wave_text_bytes / 1e9,
                    g.find_ms, g.decode_ms, g.resolve_ms);
        }
    }
    if (R.flags) {
        *irregular = (int)R.flags;
        return RALA_HIP_OK;
    }
    if (R.first_bad != ~0ull) {
        *length_error_read = (int64_t)(R.first_bad & 0xFFFFFFFFull);
        return RALA_HIP_OK;
    }
    rala_hip_overlaps dev;
    dev.a_id = ctx->d_paf_col[0].p; dev.b_id = ctx->d_paf_col[1].p; dev.a_begin = ctx->d_paf_col[2].p; dev.a_end = ctx->d_paf_col[3].p;
    dev.b_begin = ctx->d_paf_col[4].p; dev.b_end = ctx->d_paf_col[5].p; dev.length = ctx->d_paf_col[6].p; dev.strand = ctx->d_paf_strand.p;
    return rala_hip_set_overlaps(ctx, &dev, R.n_lines, RALA_HIP_MEM_DEVICE);
}

// The sensitive overlaps (-s; Graph::preprocess, graph.cpp:901-939) of an uncompressed PAF file tokenised on the device, no
// length check (Overlap::transmute_ has none, overlap.cpp:84-114): bytes [lo, hi) of the file's lines (hi = ~0: to its end; a
// rank of a sharded run takes a share - any split of the sensitive set will do).  out: device pointers that stay the
// context's (valid until the next call); hand them to rala_hip_construct / rala_hip_mg_run with the option
// "sensitive_in_device_memory" set.  *irregular != 0: not a file of 12-column records, nothing was set - take the host reader.
int rala_hip_tokenise_sensitive_paf(rala_hip_ctx* ctx, const char* path, uint64_t lo, uint64_t hi, uint32_t threads, rala_hip_overlaps* out,
                                    uint64_t* n, int* irregular) {
    if (!ctx || !path || !out || !n || !irregular) return RALA_HIP_EINVAL;
    *irregular = 0;
    *n = 0;
    PafTarget T;
    for (int k = 0; k < 7; ++k) T.col[k] = &ctx->d_sens_col[k];
    T.strand = &ctx->d_sens_strand;
    PafRange R;
    const int rc = paf_tokenise_range(ctx, path, lo, hi, false, threads, 0, T, &R);
    if (rc != RALA_HIP_OK) return rc;
    if (R.flags) { *irregular = (int)R.flags; return RALA_HIP_OK; }
    out->a_id = ctx->d_sens_col[0].p; out->b_id = ctx->d_sens_col[1].p; out->a_begin = ctx->d_sens_col[2].p; out->a_end = ctx->d_sens_col[3].p;
    out->b_begin = ctx->d_sens_col[4].p; out->b_end = ctx->d_sens_col[5].p; out->length = ctx->d_sens_col[6].p; out->strand = ctx->d_sens_strand.p;
    *n = R.n_lines;
    return RALA_HIP_OK;
}

int rala_hip_get_overlap_columns(rala_hip_ctx* ctx, uint64_t* n, uint32_t* const cols[7], uint8_t* strand) {
    if (!ctx || !n) return RALA_HIP_EINVAL;
    if (!ctx->inputs_set || ctx->tuple_mode) return ingest_fail(ctx, RALA_HIP_EINVAL, "no overlaps set");
    *n = ctx->n_ovl;
    if (!cols && !strand) return RALA_HIP_OK;
    INGEST_CHECK(hipSetDevice(ctx->device));
    { const int rcu = rala_hip::flush_upload(ctx); if (rcu != RALA_HIP_OK) return rcu; }
    const uint32_t* src[7] = {ctx->ovl.a_id, ctx->ovl.b_id, ctx->ovl.a_begin, ctx->ovl.a_end, ctx->ovl.b_begin, ctx->ovl.b_end, ctx->ovl.length};
    for (int k = 0; cols && k < 7; ++k) {
        if (cols[k] && ctx->n_ovl) INGEST_CHECK(hipMemcpy(cols[k], src[k], ctx->n_ovl * 4, hipMemcpyDeviceToHost));
    }
    if (strand && ctx->n_ovl) INGEST_CHECK(hipMemcpy(strand, ctx->ovl.strand, ctx->n_ovl, hipMemcpyDeviceToHost));
    return RALA_HIP_OK;
}

int rala_hip_index_sequences(rala_hip_ctx* ctx, const char* path, int format, uint32_t threads, uint64_t* n_records, uint64_t* name_bytes,
                             int* irregular) {
    if (!ctx || !path || !n_records || !name_bytes || !irregular || (format != 0 && format != 1)) return RALA_HIP_EINVAL;
    *n_records = *name_bytes = 0;
    *irregular = 0;
    ctx->seq_index_valid = false;
    ctx->n_seq_records = ctx->n_seq_name_bytes = 0;
    ctx->seq_tm = rala_hip_ingest_timings();
    INGEST_CHECK(hipSetDevice(ctx->device));
    Fd file;
    file.fd = open(path, O_RDONLY);
    if (file.fd < 0) return ingest_fail(ctx, RALA_HIP_EINVAL, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(file.fd, &st) != 0 || !S_ISREG(st.st_mode)) return ingest_fail(ctx, RALA_HIP_ENOTAFILE, std::string("not a regular file: ") + path);
    const uint64_t file_n = (uint64_t)st.st_size;
    // the window over the text: the overlap ingest's rule, and every count of a window in 32 bits.  A gzip file: BGZF is
    // inflated on the device, so is (option gzip_on_device) any other file of one member; what is left is the host reader's
    TextSource S;
    S.fd = file.fd;
    S.path = path;
    S.threads = threads;
    S.file_n = file_n;
    {
        bool valid = true;
        const int rc = source_open(ctx, S, ctx->gzip_on_device, nullptr, &valid);
        if (S.gz) ctx->gzip_tm = S.gz->tm;
        if (rc != RALA_HIP_OK || !valid) {
            source_close(ctx);
            if (rc != RALA_HIP_OK) return rc;
            *irregular = 8;
            return RALA_HIP_OK;
        }
    }
    SequenceRun R;
    R.fastq = format == 1;
    R.text_n = S.text_n;
    hipStream_t s = ctx->stream;
    double kernel_ms = 0;
    uint32_t flags = 0;
    int rc = RALA_HIP_OK;
    // (a gzip member is inflated to its end even where the index has given up: CRC32 and ISIZE say whether that was its text)
    while (S.lo < R.text_n && rc == RALA_HIP_OK && !S.flag && (!flags || S.gz)) {
        TextWindow w;
        rc = source_next(ctx, S, &w);
        if (rc != RALA_HIP_OK || S.flag) break;
        if (!flags) rc = index_window(ctx, R, w.text, w.lo, w.n, w.n_avail, &flags);
        if (rc == RALA_HIP_OK) rc = source_advance(ctx, S, w);
        kernel_ms += now_ms() - w.t_kernels;
    }
    if (S.gz) {
        ctx->gzip_tm = S.gz->tm;
        if (rc == RALA_HIP_OK && !S.flag && !gzip_walk_proven(*S.gz)) S.flag = 8;
        if (getenv("RALA_HIP_TRACE")) trace_gzip_walk(*S.gz);
    }
    if (S.flag) flags = 8;
    const double ship_ms = S.ship_ms;
    source_close(ctx);
    if (rc != RALA_HIP_OK) return rc;
    if (!flags && R.fastq && (R.n_events & 3u) != 0) flags = kSeqNotFourLines;       // a record cut after 1, 2 or 3 lines
    const double tf = now_ms();
    std::vector<uint32_t> length(R.n_records);
    if (!flags && R.n_records) {
        if (ctx->d_seq_span.ensure(R.n_records) != hipSuccess || ctx->d_seq_length.ensure(R.n_records) != hipSuccess) {
            return ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the sequence index");
        }
        SequenceColumns C;
        C.event_pos = ctx->d_seq_event[0].p; C.event_stripped = ctx->d_seq_event[1].p;
        C.name_pos = ctx->d_seq_name_pos.p; C.name_len = ctx->d_seq_name_len.p;
        C.data_off = ctx->d_seq_data_off.p; C.data_stripped = ctx->d_seq_data_stripped.p;
        INGEST_CHECK(hipMemsetAsync(ctx->d_seq_flags.p, 0, 4, s));
        launch_sequence_finish(R.n_records, R.n_events, R.text_n, R.n_stripped, R.fastq, C, ctx->d_seq_span.p, ctx->d_seq_length.p, ctx->d_seq_flags.p, s);
        INGEST_CHECK(hipGetLastError());
        INGEST_CHECK(hipMemcpyAsync(&flags, ctx->d_seq_flags.p, 4, hipMemcpyDeviceToHost, s));
        INGEST_CHECK(hipMemcpyAsync(length.data(), ctx->d_seq_length.p, R.n_records * 4, hipMemcpyDeviceToHost, s));
        INGEST_CHECK(hipStreamSynchronize(s));
    }
    kernel_ms += now_ms() - tf;
    ctx->seq_tm.ship_ms = (float)ship_ms;
    ctx->seq_tm.tokenize_ms = (float)kernel_ms;
    ctx->seq_tm.bytes = R.text_n;
    ctx->seq_tm.lines = R.n_records;
    if (getenv("RALA_HIP_TRACE")) {
        fprintf(stderr, "[trace] device sequence index: %.2f GB of text shipped in %.1f ms, %lu records indexed in %.2f ms (flags %u)\n", R.text_n / 1e9,
                ship_ms, (unsigned long)R.n_records, kernel_ms, flags);
    }
    if (flags & kSeqTooLong) return ingest_fail(ctx, RALA_HIP_ETOOLARGE, "a sequence of 2^32 bases or more");
    if (flags) {
        *irregular = (int)flags;
        return RALA_HIP_OK;
    }
    // the lengths are the context's reads from here on
    const int rcr = rala_hip_set_reads(ctx, length.data(), R.n_records);
    if (rcr != RALA_HIP_OK) return rcr;
    ctx->n_seq_records = R.n_records;
    ctx->n_seq_name_bytes = R.name_bytes;
    ctx->seq_index_valid = true;
    ctx->seq_source = S.kind;
    ctx->seq_fastq = R.fastq;
    ctx->seq_file_n = file_n;
    ctx->seq_text_n = R.text_n;
    ctx->seq_n_stripped = R.n_stripped;
    ctx->seq_gzip_chain.clear();
    if (S.gz) {
        ctx->seq_gzip_chain.swap(S.gz->chain);
        ctx->seq_gzip_crc = S.gz->crc;
    }
    *n_records = R.n_records;
    *name_bytes = R.name_bytes;
    return RALA_HIP_OK;
}

int rala_hip_get_sequence_index(rala_hip_ctx* ctx, uint64_t* name_off, uint32_t* name_len, uint64_t* data_off, uint64_t* data_span,
                                uint32_t* length, char* names) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (!ctx->seq_index_valid) return ingest_fail(ctx, RALA_HIP_EINVAL, "no sequence index (rala_hip_index_sequences)");
    INGEST_CHECK(hipSetDevice(ctx->device));
    const uint64_t n = ctx->n_seq_records;
    if (n && name_off) INGEST_CHECK(hipMemcpy(name_off, ctx->d_seq_name_off.p, n * 8, hipMemcpyDeviceToHost));
    if (n && name_len) INGEST_CHECK(hipMemcpy(name_len, ctx->d_seq_name_len.p, n * 4, hipMemcpyDeviceToHost));
    if (n && data_off) INGEST_CHECK(hipMemcpy(data_off, ctx->d_seq_data_off.p, n * 8, hipMemcpyDeviceToHost));
    if (n && data_span) INGEST_CHECK(hipMemcpy(data_span, ctx->d_seq_span.p, n * 8, hipMemcpyDeviceToHost));
    if (n && length) INGEST_CHECK(hipMemcpy(length, ctx->d_seq_length.p, n * 4, hipMemcpyDeviceToHost));
    if (ctx->n_seq_name_bytes && names) INGEST_CHECK(hipMemcpy(names, ctx->d_seq_arena.p, ctx->n_seq_name_bytes, hipMemcpyDeviceToHost));
    return RALA_HIP_OK;
}

int rala_hip_get_sequence_timings(rala_hip_ctx* ctx, rala_hip_ingest_timings* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->seq_tm;
    return RALA_HIP_OK;
}

int rala_hip_slice_sequences(rala_hip_ctx* ctx, const char* path, const uint64_t* wanted, uint64_t n_wanted, const uint64_t* base_off,
                             uint8_t* bases, uint32_t threads, int* irregular) {
    if (!ctx || !path || !irregular || !base_off || (n_wanted && !wanted) || (!bases && base_off[n_wanted])) return RALA_HIP_EINVAL;
    *irregular = 0;
    ctx->slice_info = rala_hip_sequence_slice_info();
    if (!ctx->seq_index_valid) { *irregular = 64; return RALA_HIP_OK; }
    INGEST_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n_rec = ctx->n_seq_records;
    // what the index holds of the wanted reads (none of them empty): where their text lies, where their bases go
    std::vector<uint64_t> data_off(n_rec), span(n_rec), data_stripped(n_rec);
    std::vector<uint32_t> length(n_rec);
    if (n_rec) {
        INGEST_CHECK(hipMemcpy(data_off.data(), ctx->d_seq_data_off.p, n_rec * 8, hipMemcpyDeviceToHost));
        INGEST_CHECK(hipMemcpy(span.data(), ctx->d_seq_span.p, n_rec * 8, hipMemcpyDeviceToHost));
        INGEST_CHECK(hipMemcpy(data_stripped.data(), ctx->d_seq_data_stripped.p, n_rec * 8, hipMemcpyDeviceToHost));
        INGEST_CHECK(hipMemcpy(length.data(), ctx->d_seq_length.p, n_rec * 4, hipMemcpyDeviceToHost));
    }
    std::vector<uint64_t> w_off, w_end, w_adj, w_base;
    if (base_off[0] != 0) return ingest_fail(ctx, RALA_HIP_EINVAL, "base_off does not begin at 0");
    for (uint64_t k = 0; k < n_wanted; ++k) {
        const uint64_t r = wanted[k];
        if (r >= n_rec || (k && r <= wanted[k - 1])) return ingest_fail(ctx, RALA_HIP_EINVAL, "wanted reads not ascending records of the index");
        if (base_off[k + 1] - base_off[k] != length[r]) return ingest_fail(ctx, RALA_HIP_EINVAL, "base_off is not the scan of the wanted reads' lengths");
        if (!length[r]) continue;
        w_off.push_back(data_off[r]);
        w_end.push_back(data_off[r] + span[r]);
        w_adj.push_back(base_off[k] - data_off[r] + data_stripped[r]);
        w_base.push_back(base_off[k]);
    }
    const uint64_t n_w = w_off.size(), n_bases = base_off[n_wanted];
    Fd file;
    file.fd = open(path, O_RDONLY);
    struct stat st;
    if (file.fd < 0 || fstat(file.fd, &st) != 0 || !S_ISREG(st.st_mode) || (uint64_t)st.st_size != ctx->seq_file_n) { *irregular = 64; return RALA_HIP_OK; }
    if (!n_w) return RALA_HIP_OK;
    // whatever way this call ends, the wanted reads, a window's bases and the source's buffers do not stay the context's
    struct Release {
        rala_hip_ctx* ctx;
        ~Release() {
            source_close(ctx);
            ctx->d_slice_out.release();
            for (int k = 0; k < 3; ++k) ctx->d_slice_w[k].release();
        }
    } release{ctx};
    for (int k = 0; k < 3; ++k) INGEST_CHECK(ctx->d_slice_w[k].ensure(n_w));
    INGEST_CHECK(hipMemcpy(ctx->d_slice_w[0].p, w_off.data(), n_w * 8, hipMemcpyHostToDevice));
    INGEST_CHECK(hipMemcpy(ctx->d_slice_w[1].p, w_end.data(), n_w * 8, hipMemcpyHostToDevice));
    INGEST_CHECK(hipMemcpy(ctx->d_slice_w[2].p, w_adj.data(), n_w * 8, hipMemcpyHostToDevice));
    TextSource S;
    S.fd = file.fd;
    S.path = path;
    S.threads = threads;
    S.file_n = (uint64_t)st.st_size;
    {
        bool valid = true;
        const int rc = source_open(ctx, S, ctx->seq_source == 2, ctx->seq_source == 2 ? &ctx->seq_gzip_chain : nullptr, &valid);
        if (rc != RALA_HIP_OK || !valid || S.kind != ctx->seq_source || S.text_n != ctx->seq_text_n ||
            (S.gz && (S.gz->crc != ctx->seq_gzip_crc || S.gz->chain.back().stop_bit != kGzipNoStart))) {
            if (rc != RALA_HIP_OK) return rc;
            *irregular = valid && S.kind == ctx->seq_source && !S.gz ? 64 : 8;
            return RALA_HIP_OK;
        }
    }
    const uint64_t tile = sequence_tile_bytes();
    uint64_t n_stripped = 0, k_lo = 0;
    bool last_is_newline = true;
    double kernel_ms = 0, gather_ms = 0, copy_ms = 0;
    uint32_t flags = 0;
    int rc = RALA_HIP_OK;
    INGEST_CHECK(ctx->d_seq_flags.ensure(1));
    INGEST_CHECK(hipMemsetAsync(ctx->d_seq_flags.p, 0, 4, s));
    // (a gzip member is inflated to its end, wanted reads or not: a window's markers point into the one before, and CRC32
    // and ISIZE say at the end whether this was the text the index saw)
    while (S.lo < S.text_n && rc == RALA_HIP_OK && !S.flag && !flags && (k_lo < n_w || S.gz)) {
        TextWindow w;
        rc = source_next(ctx, S, &w);
        if (rc != RALA_HIP_OK || S.flag) break;
        const uint64_t n_tiles = (w.n + tile - 1) / tile;
        if (n_tiles && k_lo < n_w) {
            // the stripped bytes in front of every tile, as the index counted them
            if (ctx->d_seq_tile[0].ensure(n_tiles + 2) != hipSuccess || ctx->d_seq_tile[1].ensure(n_tiles + 2) != hipSuccess ||
                ctx->d_scan_ws.ensure(scan_workspace_bytes(n_tiles + 2)) != hipSuccess) {
                rc = ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for the tiles' counts");
                break;
            }
            launch_sequence_count(w.text, w.n, last_is_newline, ctx->seq_fastq, ctx->d_seq_tile[0].p, ctx->d_seq_tile[1].p, s);
            launch_exclusive_scan(ctx->d_seq_tile[1].p, ctx->d_seq_tile[1].p, n_tiles, ctx->d_scan_ws.p, s);
            uint32_t stripped = 0;
            uint8_t last = 0;
            if (hipMemcpyAsync(&stripped, ctx->d_seq_tile[1].p + n_tiles, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(&last, w.text + w.n - 1, 1, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
                rc = ingest_fail(ctx, RALA_HIP_EDEVICE, "counting a window's stripped bytes failed");
                break;
            }
            // the wanted reads with text in [lo, hi), and the share of the output that is this window's
            const uint64_t lo = w.lo, hi = w.lo + w.n;
            while (k_lo < n_w && w_end[k_lo] <= lo) ++k_lo;
            const uint64_t k_hi = std::lower_bound(w_off.begin() + k_lo, w_off.end(), hi) - w_off.begin();
            if (k_lo < k_hi) {
                const uint64_t out_lo = w_off[k_lo] >= lo ? w_base[k_lo] : lo - n_stripped + w_adj[k_lo];
                const uint64_t out_hi = w_end[k_hi - 1] <= hi ? (k_hi < n_w ? w_base[k_hi] : n_bases) : hi - (n_stripped + stripped) + w_adj[k_hi - 1];
                if (out_hi < out_lo || out_hi > n_bases || out_hi - out_lo > w.n) { flags = kSeqSliceMismatch; break; }
                const uint64_t out_n = out_hi - out_lo;
                if (out_n) {
                    if (ctx->d_slice_out.ensure(out_n) != hipSuccess) { rc = ingest_fail(ctx, RALA_HIP_ENOMEM, "device memory for a window's bases"); break; }
                    SequenceGather G;
                    G.text = w.text; G.n = w.n; G.text_off = lo;
                    G.tile_stripped0 = ctx->d_seq_tile[1].p; G.stripped0 = n_stripped;
                    G.w_off = ctx->d_slice_w[0].p; G.w_end = ctx->d_slice_w[1].p; G.w_adj = ctx->d_slice_w[2].p;
                    G.k_lo = k_lo; G.k_hi = k_hi;
                    G.out_lo = out_lo; G.out_n = out_n; G.out = ctx->d_slice_out.p; G.flags = ctx->d_seq_flags.p;
                    const double tg = now_ms();
                    launch_sequence_gather(G, s);
                    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { rc = ingest_fail(ctx, RALA_HIP_EDEVICE, "the gather kernel failed"); break; }
                    const double tc = now_ms();
                    if (hipMemcpyAsync(bases + out_lo, ctx->d_slice_out.p, out_n, hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipMemcpyAsync(&flags, ctx->d_seq_flags.p, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
                        rc = ingest_fail(ctx, RALA_HIP_EDEVICE, "copying a window's bases failed");
                        break;
                    }
                    gather_ms += tc - tg;
                    copy_ms += now_ms() - tc;
                    ctx->slice_info.bases += out_n;
                }
            }
            n_stripped += stripped;
            last_is_newline = last == '\n';
        }
        if (rc == RALA_HIP_OK) rc = source_advance(ctx, S, w);
        kernel_ms += now_ms() - w.t_kernels;
    }
    if (S.gz && rc == RALA_HIP_OK && !S.flag && !flags && !gzip_walk_proven(*S.gz)) S.flag = 8;
    if (S.gz) ctx->gzip_tm = S.gz->tm;
    if (rc != RALA_HIP_OK) return rc;
    if (!S.flag && !flags && ctx->slice_info.bases != n_bases) flags = kSeqSliceMismatch;
    ctx->slice_info.windows = S.windows;
    ctx->slice_info.max_window_text_bytes = S.max_window;
    ctx->slice_info.ship_ms = (float)S.ship_ms;
    ctx->slice_info.kernel_ms = (float)kernel_ms;
    ctx->slice_info.gather_ms = (float)gather_ms;
    ctx->slice_info.copy_ms = (float)copy_ms;
    if (getenv("RALA_HIP_TRACE")) {
        fprintf(stderr, "[trace] device sequence slice: %lu windows of at most %.3f GB of text, %lu bases of %lu reads, ship %.1f ms, device %.2f ms "
                "(gather %.2f ms, bases to the host %.2f ms) (flags %u)\n", (unsigned long)S.windows, S.max_window / 1e9,
                (unsigned long)ctx->slice_info.bases, (unsigned long)n_wanted, S.ship_ms, kernel_ms, gather_ms, copy_ms, S.flag | flags);
    }
    if (S.flag || flags) *irregular = (int)(S.flag | flags);
    return RALA_HIP_OK;
}

int rala_hip_get_sequence_slice_info(rala_hip_ctx* ctx, rala_hip_sequence_slice_info* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->slice_info;
    return RALA_HIP_OK;
}

uint32_t rala_hip_crc32_chain(const uint32_t* reg, const uint64_t* len, uint64_t n) {
    if (n && (!reg || !len)) return 0;
    return gzip_crc_chain(reg, len, n);
}

int rala_hip_get_ingest_timings(rala_hip_ctx* ctx, rala_hip_ingest_timings* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->ingest_tm;
    return RALA_HIP_OK;
}

int rala_hip_get_inflate_timings(rala_hip_ctx* ctx, rala_hip_inflate_timings* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->inflate_tm;
    return RALA_HIP_OK;
}

int rala_hip_get_gzip_timings(rala_hip_ctx* ctx, rala_hip_gzip_timings* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->gzip_tm;
    return RALA_HIP_OK;
}

int rala_hip_gzip_head(const uint8_t* bytes, uint64_t n, uint64_t* deflate_off, int* valid) {
    if ((!bytes && n) || !deflate_off || !valid) return RALA_HIP_EINVAL;
    *deflate_off = 0;
    *valid = gzip_head(bytes, n, deflate_off) ? 1 : 0;
    return RALA_HIP_OK;
}

int rala_hip_bgzf_index(const uint8_t* bytes, uint64_t n, uint64_t block_bytes, uint64_t cap, uint64_t* n_members, uint64_t* file_off,
                        uint32_t* comp_bytes, uint32_t* text_bytes, uint64_t* text_off, int* valid) {
    if ((!bytes && n) || !n_members || !valid) return RALA_HIP_EINVAL;
    std::vector<BgzfMember> m;
    *valid = bgzf_index_bytes(bytes, n, block_bytes ? block_bytes : kBlockBytes, m) ? 1 : 0;
    *n_members = *valid ? m.size() : 0;
    if (!*valid || cap < m.size()) return RALA_HIP_OK;
    for (size_t i = 0; i < m.size(); ++i) {
        if (file_off) file_off[i] = m[i].off;
        if (comp_bytes) comp_bytes[i] = m[i].bsize;
        if (text_bytes) text_bytes[i] = m[i].isize;
        if (text_off) text_off[i] = m[i].text_off;
    }
    return RALA_HIP_OK;
}

}  // extern "C"
