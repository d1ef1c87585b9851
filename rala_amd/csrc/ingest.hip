// Host side of the device tokeniser (ingest_kernels.hip): the file's text to device memory (ingest_ship.hip; inflated there
// where the file is BGZF or one gzip member: ingest_bgzf.hip, ingest_gzip.hip), then count, scan, parse, and the columns
// become the context's overlaps (rala_hip_set_overlaps, device memory).
#include "ingest_common.h"
#include "lifecycle.h"
#include "name_table.h"

using namespace rala_hip;
using namespace rala_hip::ingest;

namespace {

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
    const bool trace = trace_on();
    double tc = t1, tp0 = t1, tp1 = t1;
    uint32_t n_lines = 0;
    if (n_chunks) {
        launch_paf_count(text, n, first_is_start, ctx->d_paf_chunk[0].p, s);
        launch_exclusive_scan(ctx->d_paf_chunk[0].p, ctx->d_paf_chunk[1].p, n_chunks, ctx->d_scan_ws.p, s);
        HIPCHECK(hipMemcpyAsync(&n_lines, ctx->d_paf_chunk[1].p + n_chunks, 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
    }
    tc = now_ms();
    if ((uint64_t)n_lines >= 0xFFFFFFF0ull / 2) return fail(ctx, RALA_HIP_ETOOLARGE, "too many overlaps for 32-bit bound offsets");
    for (int k = 0; k < 7; ++k) HIPCHECK(T.col[k]->ensure((size_t)n_lines + 1 + extra_rows));
    HIPCHECK(T.strand->ensure((size_t)n_lines + 1 + extra_rows));
    unsigned long long bad = ~0ull;
    uint32_t flags = 0;
    if (n_lines) {
        tp0 = now_ms();
        HIPCHECK(hipMemsetAsync(ctx->d_paf_bad.p, 0xFF, 8, s));
        HIPCHECK(hipMemsetAsync(ctx->d_paf_bad.p + 1, 0, 8, s));
        PafColumns cols;
        cols.a_id = T.col[0]->p; cols.b_id = T.col[1]->p; cols.a_begin = T.col[2]->p; cols.a_end = T.col[3]->p;
        cols.b_begin = T.col[4]->p; cols.b_end = T.col[5]->p; cols.length = T.col[6]->p; cols.strand = T.strand->p;
        launch_paf_parse(text, n, n_avail, first_is_start, ctx->d_paf_chunk[1].p, ctx->d_name_buckets.p, std::max<uint64_t>(ctx->n_name_buckets, 1),
                         (const char*)ctx->d_name_arena.p, ctx->d_read_len.p, (uint32_t)ctx->n_reads, check_lengths, cols,
                         (uint32_t*)(ctx->d_paf_bad.p + 1), ctx->d_paf_bad.p, s, T.mhap);
        unsigned long long back[2] = {0, 0};
        HIPCHECK(hipMemcpyAsync(back, ctx->d_paf_bad.p, 16, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        HIPCHECK(hipGetLastError());
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

PafTarget paf_target(DevBuf<uint32_t>* col, DevBuf<uint8_t>* strand, bool mhap) {
    PafTarget T;
    for (int k = 0; k < 7; ++k) T.col[k] = &col[k];
    T.strand = strand;
    T.mhap = mhap;
    return T;
}

// An overlap file's text, wherever it comes from: a plain file's bytes, a BGZF file's members (text_n: their text), a gzip
// member's text resident in ctx->d_gzip_text.
struct OverlapText {
    TextKind kind = kTextPlain;
    Fd file;
    const char* path = nullptr;
    uint64_t file_n = 0, text_n = 0;
    BgzfFile bg;
    GzipStream gz;
    uint32_t n_readers = 0;             // of the last range
};

// the byte in front of text position lo (> 0): the file's for a plain file, else the one in front of `text` in device memory
int byte_before(rala_hip_ctx* ctx, const OverlapText& X, const uint8_t* text, uint64_t lo, uint8_t* before) {
    if (X.kind != kTextPlain) HIPCHECK(hipMemcpy(before, text - 1, 1, hipMemcpyDeviceToHost));
    else if (pread(X.file.fd, before, 1, (off_t)(lo - 1)) != 1) return fail(ctx, RALA_HIP_EDEVICE, std::string("reading ") + X.path + " failed");
    return RALA_HIP_OK;
}

// The text [lo, lo + n_avail) in device memory with cap - n_avail newlines behind it, and (lo > 0) the byte in front of it;
// meanwhile (the tokeniser's memory) runs while the readers work, where there are any (resident text: in front of its arrival).
int overlap_text_range(rala_hip_ctx* ctx, OverlapText& X, uint64_t lo, uint64_t n_avail, uint64_t cap, uint32_t threads,
                       const std::function<bool()>& meanwhile, TextArrival* out, uint8_t* before) {
    const char* const room = "device memory for the overlap columns";
    if (X.kind == kTextBgzf) {
        const int rc = bgzf_text_range(ctx, X.bg, lo, n_avail, cap, '\n', threads, meanwhile, room, out);
        X.n_readers = X.bg.n_readers;
        return rc != RALA_HIP_OK || out->flag || !lo ? rc : byte_before(ctx, X, out->text, lo, before);
    }
    if (X.kind == kTextGzip) {
        if (!meanwhile()) return fail(ctx, RALA_HIP_ENOMEM, room);
        out->text = ctx->d_gzip_text.p + lo;
        X.n_readers = X.gz.n_readers;
        const int rc = lo ? byte_before(ctx, X, out->text, lo, before) : RALA_HIP_OK;
        out->t0 = out->t_ship = out->t1 = now_ms();
        return rc;
    }
    if (lo) { const int rc = byte_before(ctx, X, nullptr, lo, before); if (rc != RALA_HIP_OK) return rc; }
    hipStream_t s = ctx->stream;
    out->t0 = now_ms();
    if (ctx->d_paf_text.ensure(cap) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the file's text");
    HIPCHECK(hipMemsetAsync(ctx->d_paf_text.p + n_avail, '\n', cap - n_avail, s));
    const int shipped = ship_file(X.file.fd, lo, n_avail, ctx->d_paf_text.p, ctx->device, threads, nullptr, meanwhile, &X.n_readers);
    if (shipped == 2) return fail(ctx, RALA_HIP_ENOMEM, room);
    if (shipped) return fail(ctx, RALA_HIP_EDEVICE, std::string("reading / copying ") + X.path + " failed");
    HIPCHECK(hipStreamSynchronize(s));
    out->text = ctx->d_paf_text.p;
    out->t_ship = out->t1 = now_ms();
    return RALA_HIP_OK;
}

// The lines that START in bytes [lo, hi) of the text (hi = ~0: to its end), tokenised on the device into `T`'s columns (room for
// extra_rows more rows than the range holds: a rank of a sharded run receives the heads of its neighbours' first runs), with
// what the last lines' first eleven columns may need behind hi.
int tokenise_range(rala_hip_ctx* ctx, OverlapText& X, uint64_t lo, uint64_t hi, bool check_lengths, uint32_t threads, size_t extra_rows,
                   const PafTarget& T, PafRange* out) {
    *out = PafRange();
    hi = std::min(hi, X.text_n);
    lo = std::min(lo, hi);
    const uint64_t n = hi - lo;                                             // bytes whose line starts are ours
    const uint64_t n_avail = std::min<uint64_t>(X.text_n - lo, n + paf_halo_bytes());
    const uint32_t chunk = paf_chunk_bytes();
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    if (n_chunks >= 0xFFFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "file too large for 32-bit chunk ids");
    const uint64_t cap = n_chunks * chunk + 4096 + 64;
    TextArrival A;
    uint8_t before = '\n';
    const int rc = overlap_text_range(ctx, X, lo, n_avail, cap, threads, [&]() { return tokeniser_memory(ctx, n, n_chunks, extra_rows, T); }, &A, &before);
    if (rc != RALA_HIP_OK) return rc;
    if (A.flag) { out->flags = A.flag; return RALA_HIP_OK; }
    out->file_bytes = X.file_n;
    return tokenise_text(ctx, A.text, n, n_avail, before == '\n', check_lengths, extra_rows, T, out, A.t1 - (A.t_ship - A.t0), A.t1, X.n_readers);
}

}  // namespace

// tokenise_range of an uncompressed file
int rala_hip::paf_tokenise_range(rala_hip_ctx* ctx, const char* path, uint64_t lo, uint64_t hi, bool check_lengths, uint32_t threads,
                                 size_t extra_rows, const PafTarget& T, PafRange* out) {
    if (!ctx || !path || !out) return RALA_HIP_EINVAL;
    *out = PafRange();
    int rc = ingest_ready(ctx, T.mhap);
    if (rc != RALA_HIP_OK) return rc;
    HIPCHECK(hipSetDevice(ctx->device));
    OverlapText X;
    X.path = path;
    rc = open_regular(ctx, path, X.file, &X.file_n);
    if (rc != RALA_HIP_OK) return rc;
    X.text_n = X.file_n;
    return tokenise_range(ctx, X, lo, hi, check_lengths, threads, extra_rows, T, out);
}

int rala_hip::overlap_tokenise_part(rala_hip_ctx* ctx, const char* path, uint32_t part, uint32_t parts, const PartKinds& take, bool check_lengths,
                                    uint32_t threads, size_t extra_rows, const PafTarget& T, PafRange* out, uint64_t piece[3], bool* bgzf) {
    if (!ctx || !path || !out || !piece || !bgzf || parts == 0 || part >= parts) return RALA_HIP_EINVAL;
    *out = PafRange();
    *bgzf = false;
    piece[0] = piece[1] = 0;
    piece[2] = 1;
    int rc = ingest_ready(ctx, T.mhap);
    if (rc != RALA_HIP_OK) return rc;
    HIPCHECK(hipSetDevice(ctx->device));
    OverlapText X;
    X.path = path;
    rc = open_regular(ctx, path, X.file, &X.file_n);
    if (rc != RALA_HIP_OK) return rc;
    X.text_n = X.file_n;
    uint8_t head[18] = {0};
    const ssize_t got = pread(X.file.fd, head, sizeof(head), 0);
    X.kind = sniff(head, (uint64_t)std::max<ssize_t>(got, 0));
    const bool taken = (X.kind == kTextBgzf && take.bgzf_pieces) || (X.kind == kTextGzip && take.gzip_whole && parts == 1 && ctx->gzip_on_device);
    if (X.kind != kTextPlain && !taken) {
        if (take.refuse_other) { out->flags = 8; return RALA_HIP_OK; }
        X.kind = kTextPlain;
    }
    const uint64_t F = X.file_n;
    const uint64_t lo = F / parts * part + std::min<uint64_t>(part, F % parts), hi = F / parts * (part + 1) + std::min<uint64_t>(part + 1, F % parts);
    if (X.kind == kTextPlain) {
        piece[0] = lo; piece[1] = hi; piece[2] = 0;
        return tokenise_range(ctx, X, lo, hi, check_lengths, threads, extra_rows, T, out);
    }
    // whatever way this ends, the compressed bytes and the inflated text do not stay the context's (it may hold piles by now)
    struct Release {
        rala_hip_ctx* ctx;
        ~Release() {
            ctx->d_bgzf_comp.release();
            ctx->d_gzip_sym.release();
            ctx->d_gzip_text.release();
            ctx->d_paf_text.release();
        }
    } release{ctx};
    bool valid = true;
    ctx->inflate_tm = rala_hip_inflate_timings();
    if (X.kind == kTextGzip) {
        X.gz.file_n = F;
        rc = gzip_inflate(ctx, X.file.fd, path, threads, X.gz, &valid);
        ctx->gzip_tm = X.gz.tm;
        if (rc != RALA_HIP_OK) return rc;
        if (!valid) { out->flags = 8; return RALA_HIP_OK; }
        X.text_n = X.gz.text_n;
        piece[0] = 0; piece[1] = F; piece[2] = 0;
        rc = tokenise_range(ctx, X, 0, ~0ull, check_lengths, threads, extra_rows, T, out);
        if (rc == RALA_HIP_OK) ctx->ingest_tm.ship_ms += X.gz.ship_ms;
        return rc;
    }
    // A BGZF piece.  Its text has no offset in the file's: positions count from the piece's first member, own of them the
    // piece's own, what follows the next members'.  A line belongs to the piece that holds the byte in front of its first
    // byte: the line starts at [1, own + 1) - position `own` is the first byte of the text that follows, inflated anyway for
    // the halo - and, the first piece's alone, the one at 0.
    *bgzf = true;
    BgzfPiece P;
    uint64_t own = 0;
    rc = bgzf_open_piece(ctx, X.file.fd, F, path, threads, lo, hi, (uint64_t)paf_halo_bytes() + 1, X.bg, &P, &own, &valid);
    piece[0] = P.begin; piece[1] = P.end; piece[2] = P.empty;
    if (rc != RALA_HIP_OK) return rc;
    if (!valid) { out->flags = 8; return RALA_HIP_OK; }
    X.text_n = X.bg.text_n;
    const bool nothing = part != 0 && own == 0;
    rc = tokenise_range(ctx, X, nothing || part == 0 ? 0 : 1, nothing ? 0 : own + 1, check_lengths, threads, extra_rows, T, out);
    if (rc != RALA_HIP_OK) return rc;
    ctx->ingest_tm.ship_ms += X.bg.ship_ms;
    ctx->inflate_tm.inflate_ms = X.bg.inflate_ms;
    ctx->inflate_tm.compressed_bytes = X.bg.shipped;
    ctx->inflate_tm.members = X.bg.jobs.size();
    if (trace_on()) {
        fprintf(stderr, "[trace] device inflate: part %u of %u, bytes [%lu, %lu) of %lu: %lu BGZF members, %.3f GB compressed shipped (index and "
                "ship %.1f ms), %.3f GB of text inflated in %.2f ms\n", part, parts, (unsigned long)P.begin, (unsigned long)P.end,
                (unsigned long)F, (unsigned long)X.bg.jobs.size(), X.bg.shipped / 1e9, X.bg.ship_ms, X.bg.text_n / 1e9, X.bg.inflate_ms);
    }
    return RALA_HIP_OK;
}

// A rank's piece of a single-member gzip file (ingest_gzip.hip: gzip_piece_*), behind the exchange of the out-windows: resolved,
// then the lines whose FIRST byte lies in the piece's own text tokenised - the rule of a plain file's byte ranges; the byte in
// front of the own text is the last of the window in front of it, the line at text offset 0 is part 0's.
int rala_hip::gzip_piece_tokenise(rala_hip_ctx* ctx, GzipPieceRun* g, const uint64_t* all, size_t stride, bool check_lengths, uint32_t threads,
                                  size_t extra_rows, const PafTarget& T, PafRange* out, uint64_t own[7]) {
    *out = PafRange();
    uint32_t flag = 0;
    int rc = gzip_piece_resolve(ctx, g, all, stride, &flag, own);
    if (rc != RALA_HIP_OK) return rc;
    if (flag) { out->flags = 8; return RALA_HIP_OK; }
    OverlapText X;
    X.kind = kTextGzip;
    uint64_t own_n = 0, n_w = 0;
    float ship_ms = 0;
    gzip_piece_text(g, &own_n, &n_w, &X.file_n, &ship_ms, &X.gz.n_readers);
    X.text_n = 16 + n_w;                        // (16 bytes in front of the text: the byte in front of it is the last of them)
    rc = tokenise_range(ctx, X, 16, 16 + own_n, check_lengths, threads, extra_rows, T, out);
    if (rc == RALA_HIP_OK) ctx->ingest_tm.ship_ms += ship_ms;
    return rc;
}

extern "C" {

int rala_hip_set_name_table(rala_hip_ctx* ctx, const void* buckets, uint64_t n_buckets, const char* arena, uint64_t arena_bytes) {
    if (!ctx || !buckets || n_buckets == 0 || (n_buckets & (n_buckets - 1)) != 0 || (!arena && arena_bytes)) return RALA_HIP_EINVAL;
    HIPCHECK(hipSetDevice(ctx->device));
    HIPCHECK(ctx->d_name_buckets.ensure(n_buckets * sizeof(NameBucket)));
    HIPCHECK(ctx->d_name_arena.ensure(arena_bytes + 16));
    HIPCHECK(hipMemcpy(ctx->d_name_buckets.p, buckets, n_buckets * sizeof(NameBucket), hipMemcpyHostToDevice));
    if (arena_bytes) HIPCHECK(hipMemcpy(ctx->d_name_arena.p, arena, arena_bytes, hipMemcpyHostToDevice));
    ctx->n_name_buckets = n_buckets;
    ctx->n_name_arena_bytes = arena_bytes;
    return RALA_HIP_OK;
}

static int set_overlaps_from_text(rala_hip_ctx* ctx, const char* path, bool mhap, int check_lengths, uint32_t threads,
                                  int64_t* length_error_read, int* irregular) {
    if (!ctx || !path || !length_error_read || !irregular) return RALA_HIP_EINVAL;
    *length_error_read = -1;
    *irregular = 0;
    // (the columns a successful call before this one left are about to be written over - whatever happens
    // here, the context has no overlaps until this call has set them)
    inputs_withdrawn(ctx);
    const PafTarget T = paf_target(ctx->d_paf_col, &ctx->d_paf_strand, mhap);
    PafRange R;
    // The file's text goes through device memory in WINDOWS (round 5; before, all of it had to fit at once): at most a
    // quarter of what is free (option ingest_window_bytes; the reference streams the file in chunks of 1 GiB,
    // graph.cpp:24, 329-365 - its run carry-over is not needed here, rows are tokenised independently of each other and
    // a window takes the lines that START in it).  One window - the usual case - tokenises straight into the columns.
    uint64_t window = (uint64_t)ctx->ingest_window_bytes;
    if (window == 0 && getenv("RALA_INGEST_WINDOW")) window = (uint64_t)atoll(getenv("RALA_INGEST_WINDOW"));      // (tests)
    HIPCHECK(hipSetDevice(ctx->device));
    window = text_window_bytes(window);
    ctx->inflate_tm = rala_hip_inflate_timings();
    ctx->gzip_tm = rala_hip_gzip_timings();
    ctx->gzip_members_last.clear();
    // A gzip file: BGZF is inflated on the device (the windows then lie over its text), so is (option gzip_on_device) any
    // other file of one member - by speculative decoding, the whole text resident afterwards, the windows over it; what is
    // left is the host reader's - known from the first 18 bytes, before anything is shipped.  (A file that cannot be opened
    // is plain text here: that refusal is decided behind the preconditions, as it ever was, and a FIFO's writer is not waited for.)
    OverlapText X;
    X.path = path;
    const int opened = open_regular(ctx, path, X.file, &X.file_n);
    uint8_t head[18] = {0};
    const ssize_t got = opened == RALA_HIP_OK ? pread(X.file.fd, head, sizeof(head), 0) : 0;
    X.kind = sniff(head, (uint64_t)std::max<ssize_t>(got, 0));
    if (X.kind == kTextGzip && !ctx->gzip_on_device) { *irregular = 8; return RALA_HIP_OK; }
    int rc = ingest_ready(ctx, mhap);
    if (rc != RALA_HIP_OK) return rc;
    if (opened != RALA_HIP_OK) return opened;           // (ctx->err is still open_regular's)
    // whatever way this call ends, the windows' columns, the compressed bytes and the inflated text do not stay the context's
    struct Release {
        rala_hip_ctx* ctx;
        ~Release() { now(); }
        void now() {
            for (int k = 0; k < 7; ++k) ctx->d_paf_win[k].release();
            ctx->d_paf_win_strand.release();
            ctx->d_bgzf_comp.release();
            ctx->d_gzip_sym.release();
            ctx->d_gzip_text.release();
        }
    } release{ctx};
    bool valid = true;
    X.text_n = X.file_n;
    if (X.kind == kTextGzip) {
        X.gz.file_n = X.file_n;
        rc = gzip_inflate(ctx, X.file.fd, path, threads, X.gz, &valid);
        ctx->gzip_tm = X.gz.tm;
        if (rc == RALA_HIP_OK && valid) ctx->gzip_members_last = X.gz.members;
        X.text_n = X.gz.text_n;
    } else if (X.kind == kTextBgzf) {
        rc = bgzf_open(ctx, X.file.fd, X.file_n, path, threads, window, X.bg, &valid);
        X.text_n = X.bg.text_n;
    }
    if (rc != RALA_HIP_OK) return rc;
    if (!valid) { *irregular = 8; return RALA_HIP_OK; }
    const uint64_t file_n = X.text_n;
    if (file_n <= window) {
        rc = tokenise_range(ctx, X, 0, ~0ull, check_lengths != 0, threads, 0, T, &R);
        if (rc != RALA_HIP_OK) return rc;
    } else {
        const PafTarget W = paf_target(ctx->d_paf_win, &ctx->d_paf_win_strand, mhap);
        uint64_t rows = 0;
        float ship = 0, tok = 0;
        for (uint64_t lo = 0; lo < file_n; lo += window) {
            PafRange part;
            rc = tokenise_range(ctx, X, lo, lo + window, check_lengths != 0, threads, 0, W, &part);
            if (rc != RALA_HIP_OK) return rc;
            ship += ctx->ingest_tm.ship_ms; tok += ctx->ingest_tm.tokenize_ms;
            R.flags |= part.flags;
            if (part.flags) break;
            if (part.first_bad != ~0ull) {          // (windows come in file order: the first one with an offender holds the first offender)
                R.first_bad = (((part.first_bad >> 32) + rows) << 32) | (part.first_bad & 0xFFFFFFFFull);
                break;
            }
            if (rows + part.n_lines >= 0xFFFFFFF0ull / 2) return fail(ctx, RALA_HIP_ETOOLARGE, "too many overlaps for 32-bit bound offsets");
            for (int k = 0; k < 7; ++k) {
                if (ctx->d_paf_col[k].grow(rows, rows + part.n_lines + 1) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the overlap columns");
                if (part.n_lines) HIPCHECK(hipMemcpy(ctx->d_paf_col[k].p + rows, ctx->d_paf_win[k].p, part.n_lines * 4, hipMemcpyDeviceToDevice));
            }
            if (ctx->d_paf_strand.grow(rows, rows + part.n_lines + 1) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the overlap columns");
            if (part.n_lines) HIPCHECK(hipMemcpy(ctx->d_paf_strand.p + rows, ctx->d_paf_win_strand.p, part.n_lines, hipMemcpyDeviceToDevice));
            rows += part.n_lines;
        }
        R.n_lines = rows;
        ctx->ingest_tm.ship_ms = ship; ctx->ingest_tm.tokenize_ms = tok;
        ctx->ingest_tm.bytes = file_n; ctx->ingest_tm.lines = rows;
    }
    if (X.kind == kTextBgzf) {
        const BgzfFile& bg = X.bg;
        ctx->ingest_tm.ship_ms += bg.ship_ms;
        ctx->inflate_tm.inflate_ms = bg.inflate_ms;
        ctx->inflate_tm.compressed_bytes = bg.shipped;
        ctx->inflate_tm.members = bg.jobs.size();
        if (trace_on()) {
            fprintf(stderr, "[trace] device inflate: %lu BGZF members, %.3f GB compressed shipped (index and ship %.1f ms), %.3f GB of text "
                    "inflated in %.2f ms\n", (unsigned long)bg.jobs.size(), bg.shipped / 1e9, bg.ship_ms, bg.text_n / 1e9, bg.inflate_ms);
        }
    }
    if (X.kind == kTextGzip) {
        ctx->ingest_tm.ship_ms += X.gz.ship_ms;
        if (trace_on()) trace_gzip(X.gz, 0, 0);
    }
    release.now();              // (not held while rala_hip_set_overlaps makes its buffers)
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

int rala_hip_set_overlaps_from_paf(rala_hip_ctx* ctx, const char* path, int check_lengths, uint32_t threads,
                                   int64_t* length_error_read, int* irregular) {
    return set_overlaps_from_text(ctx, path, false, check_lengths, threads, length_error_read, irregular);
}

int rala_hip_set_overlaps_from_mhap(rala_hip_ctx* ctx, const char* path, int check_lengths, uint32_t threads,
                                    int64_t* length_error_read, int* irregular) {
    return set_overlaps_from_text(ctx, path, true, check_lengths, threads, length_error_read, irregular);
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
    const PafTarget T = paf_target(ctx->d_sens_col, &ctx->d_sens_strand, false);
    PafRange R;
    const int rc = paf_tokenise_range(ctx, path, lo, hi, false, threads, 0, T, &R);
    if (rc != RALA_HIP_OK) return rc;
    if (R.flags) { *irregular = (int)R.flags; return RALA_HIP_OK; }
    out->a_id = ctx->d_sens_col[0].p; out->b_id = ctx->d_sens_col[1].p; out->a_begin = ctx->d_sens_col[2].p; out->a_end = ctx->d_sens_col[3].p;
    out->b_begin = ctx->d_sens_col[4].p; out->b_end = ctx->d_sens_col[5].p; out->length = ctx->d_sens_col[6].p; out->strand = ctx->d_sens_strand.p;
    *n = R.n_lines;
    return RALA_HIP_OK;
}

// The same for a share of a sensitive file of any kind (overlap_tokenise_part): plain text by byte range, BGZF by piece, any
// other gzip file whole (parts == 1, option gzip_on_device); PAF or MHAP.  piece[0 .. 2] = begin, end, empty: the caller of
// several parts joins them (rala_hip_bgzf_pieces_chain).  Only the d_sens_* columns stay.
int rala_hip_tokenise_sensitive(rala_hip_ctx* ctx, const char* path, int format, uint32_t part, uint32_t parts, uint32_t threads,
                                rala_hip_overlaps* out, uint64_t* n, uint64_t piece[3], int* irregular) {
    if (!ctx || !path || !out || !n || !piece || !irregular || (format != 0 && format != 1)) return RALA_HIP_EINVAL;
    *irregular = 0;
    *n = 0;
    const PafTarget T = paf_target(ctx->d_sens_col, &ctx->d_sens_strand, format == 1);
    PafRange R;
    PartKinds take;
    take.bgzf_pieces = take.gzip_whole = take.refuse_other = true;
    bool bgzf = false;
    const int rc = overlap_tokenise_part(ctx, path, part, parts, take, false, threads, 0, T, &R, piece, &bgzf);
    if (rc != RALA_HIP_OK) return rc;
    if (R.flags) { *irregular = (int)R.flags; return RALA_HIP_OK; }
    out->a_id = ctx->d_sens_col[0].p; out->b_id = ctx->d_sens_col[1].p; out->a_begin = ctx->d_sens_col[2].p; out->a_end = ctx->d_sens_col[3].p;
    out->b_begin = ctx->d_sens_col[4].p; out->b_end = ctx->d_sens_col[5].p; out->length = ctx->d_sens_col[6].p; out->strand = ctx->d_sens_strand.p;
    *n = R.n_lines;
    return RALA_HIP_OK;
}

int rala_hip_get_overlap_columns(rala_hip_ctx* ctx, uint64_t* n, uint32_t* const cols[7], uint8_t* strand) {
    if (!ctx || !n) return RALA_HIP_EINVAL;
    if (!ctx->inputs_set || ctx->tuple_mode) return fail(ctx, RALA_HIP_EINVAL, "no overlaps set");
    *n = ctx->n_ovl;
    if (!cols && !strand) return RALA_HIP_OK;
    HIPCHECK(hipSetDevice(ctx->device));
    { const int rcu = rala_hip::flush_upload(ctx); if (rcu != RALA_HIP_OK) return rcu; }
    const uint32_t* src[7] = {ctx->ovl.a_id, ctx->ovl.b_id, ctx->ovl.a_begin, ctx->ovl.a_end, ctx->ovl.b_begin, ctx->ovl.b_end, ctx->ovl.length};
    for (int k = 0; cols && k < 7; ++k) {
        if (cols[k] && ctx->n_ovl) HIPCHECK(hipMemcpy(cols[k], src[k], ctx->n_ovl * 4, hipMemcpyDeviceToHost));
    }
    if (strand && ctx->n_ovl) HIPCHECK(hipMemcpy(strand, ctx->ovl.strand, ctx->n_ovl, hipMemcpyDeviceToHost));
    return RALA_HIP_OK;
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

}  // extern "C"
