// The read file on the device: FASTA / FASTQ text -> names, lengths, offsets (sequence_kernels.hip), and the second pass that
// cuts the bases of the wanted reads out of the same text.
#include <memory>

#include "ingest_common.h"
#include "spell.h"

using namespace rala_hip;
using namespace rala_hip::ingest;

namespace {

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
    HIPCHECK(ctx->d_seq_tile[0].ensure(n_tiles + 2));
    HIPCHECK(ctx->d_seq_tile[1].ensure(n_tiles + 2));
    HIPCHECK(ctx->d_seq_flags.ensure(1));
    HIPCHECK(ctx->d_scan_ws.ensure(scan_workspace_bytes(n_tiles + 2)));
    launch_sequence_count(text, n, R.last_is_newline, R.fastq, ctx->d_seq_tile[0].p, ctx->d_seq_tile[1].p, s);
    launch_exclusive_scan(ctx->d_seq_tile[0].p, ctx->d_seq_tile[0].p, n_tiles, ctx->d_scan_ws.p, s);
    launch_exclusive_scan(ctx->d_seq_tile[1].p, ctx->d_seq_tile[1].p, n_tiles, ctx->d_scan_ws.p, s);
    uint32_t events = 0, stripped = 0;
    uint8_t last = 0;
    HIPCHECK(hipMemcpyAsync(&events, ctx->d_seq_tile[0].p + n_tiles, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(&stripped, ctx->d_seq_tile[1].p + n_tiles, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(&last, text + n - 1, 1, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    // (a FASTQ record is four events; one whose lines are spread over two windows is counted where its header lies)
    const uint64_t ev_after = R.n_events + events;
    const uint64_t rec_before = R.n_records, rec_after = R.fastq ? (ev_after + 3) / 4 : ev_after;
    if (ctx->d_seq_event[0].grow(R.n_events, ev_after + 1) != hipSuccess || ctx->d_seq_event[1].grow(R.n_events, ev_after + 1) != hipSuccess ||
        ctx->d_seq_name_pos.grow(rec_before, rec_after + 1) != hipSuccess || ctx->d_seq_name_len.grow(rec_before, rec_after + 1) != hipSuccess ||
        ctx->d_seq_data_off.grow(rec_before, rec_after + 1) != hipSuccess || ctx->d_seq_data_stripped.grow(rec_before, rec_after + 1) != hipSuccess ||
        ctx->d_seq_name_off.grow(rec_before, rec_after + 1) != hipSuccess) {
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for the sequence index");
    }
    HIPCHECK(hipMemsetAsync(ctx->d_seq_flags.p, 0, 4, s));
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
    HIPCHECK(hipGetLastError());
    // the headers of this window: FASTA - every event; FASTQ - the events 4r
    const uint64_t hdr_before = R.fastq ? (R.n_events + 3) / 4 : R.n_events;
    const uint64_t n_hdr = rec_after - hdr_before;
    uint32_t bytes = 0;
    if (n_hdr) {
        HIPCHECK(ctx->d_seq_name_at.ensure(n_hdr + 2));
        HIPCHECK(ctx->d_scan_ws.ensure(scan_workspace_bytes(n_hdr + 2)));
        launch_exclusive_scan(ctx->d_seq_name_len.p + hdr_before, ctx->d_seq_name_at.p, n_hdr, ctx->d_scan_ws.p, s);
        HIPCHECK(hipMemcpyAsync(&bytes, ctx->d_seq_name_at.p + n_hdr, 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipMemcpyAsync(flags, ctx->d_seq_flags.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (*flags) return RALA_HIP_OK;
    if (n_hdr) {
        if (ctx->d_seq_arena.grow(R.name_bytes, R.name_bytes + bytes + 1) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the names");
        launch_sequence_names(text, lo, ctx->d_seq_name_pos.p + hdr_before, ctx->d_seq_name_len.p + hdr_before, ctx->d_seq_name_at.p, n_hdr,
                              R.name_bytes, ctx->d_seq_arena.p, ctx->d_seq_name_off.p + hdr_before, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(s));
    }
    R.n_events = ev_after;
    R.n_stripped += stripped;
    R.n_records = rec_after;
    R.name_bytes += bytes;
    R.last_is_newline = last == '\n';
    return RALA_HIP_OK;
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
    int kind = kTextPlain;                  // TextKind
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

// *valid = false: a gzip file this does not take (not BGZF and gzip_ok false, or one the inflaters cannot prove)
int source_open(rala_hip_ctx* ctx, TextSource& S, bool gzip_ok, const std::vector<GzipJob>* chain, const std::vector<GzipMember>* members, bool* valid) {
    *valid = true;
    S.text_n = S.file_n;
    S.window = std::min<uint64_t>(text_window_bytes((uint64_t)ctx->debug_sequence_window), 1ull << 31);
    uint8_t head[18] = {0};
    const ssize_t got = pread(S.fd, head, sizeof(head), 0);
    const TextKind kind = sniff(head, (uint64_t)std::max<ssize_t>(got, 0));
    if (kind == kTextPlain) return RALA_HIP_OK;
    *valid = kind == kTextBgzf;
    if (*valid) {
        S.kind = kTextBgzf;
        S.bg.reset(new BgzfFile);
        const int rc = bgzf_open(ctx, S.fd, S.file_n, S.path.c_str(), S.threads, S.window, *S.bg, valid);
        if (rc != RALA_HIP_OK) return rc;
        S.text_n = S.bg->text_n;
        S.ship_ms = S.bg->ship_ms;
    } else if (gzip_ok) {
        S.kind = kTextGzip;
        S.gz.reset(new GzipWalk);
        S.gz->file_n = S.file_n;
        const uint64_t tile = sequence_tile_bytes(), halo = sequence_halo_bytes();
        S.front = (halo + 15) / 16 * 16;
        const int rc = gzip_walk_open(ctx, S.fd, S.path.c_str(), S.threads, (uint64_t)ctx->debug_sequence_window, S.front, tile + halo + 64 + 16, chain,
                                      members, *S.gz, valid);
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
    if (S.kind == kTextGzip) {
        uint8_t* const at = ctx->d_gzip_text.p + S.front;
        uint64_t a = 0, n_w = 0;
        const int rc = gzip_walk_next(ctx, *S.gz, at, &a, &n_w, &S.flag);
        if (rc != RALA_HIP_OK || S.flag) return rc;
        if (a != S.lo + S.hold) return fail(ctx, RALA_HIP_EDEVICE, "the gzip windows do not follow each other");
        uint8_t* text = at - S.hold;
        w->n_avail = S.hold + n_w;
        const bool last = a + n_w == S.text_n;
        w->n = last ? w->n_avail : w->n_avail > halo ? w->n_avail - halo : 0;
        const uint64_t cap = (w->n + tile - 1) / tile * tile + halo + 64;
        // What is held back is the halo, a multiple of 16, unless the windows so far were no longer than it: then all of
        // them is held back, any number of bytes, and the text in front of `at` does not begin at a multiple of 16, where
        // the index's and the slicer's kernels load it 16 bytes at a time.  Such a window goes to a buffer of its own.
        if (S.hold % 16) {
            if (ctx->d_paf_text.ensure(cap) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for a window of the inflated text");
            HIPCHECK(hipMemcpyAsync(ctx->d_paf_text.p, text, w->n_avail, hipMemcpyDeviceToDevice, s));
            text = ctx->d_paf_text.p;
        }
        HIPCHECK(hipMemsetAsync(text + w->n_avail, 0, cap - w->n_avail, s));
        HIPCHECK(hipStreamSynchronize(s));
        w->text = text;
        w->t_kernels = t0;
    } else {
        w->n = std::min(S.window, S.text_n - S.lo);
        w->n_avail = std::min<uint64_t>(S.text_n - S.lo, w->n + halo);
        const uint64_t cap = (w->n + tile - 1) / tile * tile + halo + 64;
        // what lies behind the text reads as zeros: a carriage return in the text's last byte is a base, as on the host
        if (S.kind == kTextBgzf) {
            TextArrival bt;
            const int rc = bgzf_text_range(ctx, *S.bg, S.lo, w->n_avail, cap, 0, S.threads, []() { return true; }, "device memory", &bt);
            if (rc != RALA_HIP_OK) return rc;
            if (bt.flag) { S.flag = 8; return RALA_HIP_OK; }
            w->text = bt.text;
            w->t_kernels = bt.t1;
            S.ship_ms += bt.t_ship - bt.t0;
        } else {
            if (ctx->d_paf_text.ensure(cap) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the file's text");
            if (hipMemsetAsync(ctx->d_paf_text.p + w->n_avail, 0, cap - w->n_avail, s) != hipSuccess ||
                ship_file(S.fd, S.lo, w->n_avail, ctx->d_paf_text.p, ctx->device, S.threads, nullptr, []() { return true; }, nullptr) ||
                hipStreamSynchronize(s) != hipSuccess) {
                return fail(ctx, RALA_HIP_EDEVICE, "reading / copying " + S.path + " failed");
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
    if (S.kind != kTextGzip) return RALA_HIP_OK;
    S.hold = w.n_avail - w.n;
    if (S.hold && S.lo < S.text_n) {
        hipStream_t s = ctx->stream;
        HIPCHECK(hipMemcpyAsync(ctx->d_gzip_hold.p, w.text + w.n, S.hold, hipMemcpyDeviceToDevice, s));
        HIPCHECK(hipMemcpyAsync(ctx->d_gzip_text.p + S.front - S.hold, ctx->d_gzip_hold.p, S.hold, hipMemcpyDeviceToDevice, s));
        HIPCHECK(hipStreamSynchronize(s));
    }
    return RALA_HIP_OK;
}

void source_close(rala_hip_ctx* ctx) {
    ctx->d_paf_text.release();                  // (a window of the file: not kept)
    ctx->d_bgzf_comp.release();
    ctx->d_gzip_sym.release();
    ctx->d_gzip_text.release();
}

}  // namespace

extern "C" {

int rala_hip_index_sequences(rala_hip_ctx* ctx, const char* path, int format, uint32_t threads, uint64_t* n_records, uint64_t* name_bytes,
                             int* irregular) {
    if (!ctx || !path || !n_records || !name_bytes || !irregular || (format != 0 && format != 1)) return RALA_HIP_EINVAL;
    *n_records = *name_bytes = 0;
    *irregular = 0;
    ctx->seq_index_valid = false;
    ctx->n_seq_records = ctx->n_seq_name_bytes = 0;
    ctx->seq_tm = rala_hip_ingest_timings();
    ctx->gzip_members_last.clear();
    HIPCHECK(hipSetDevice(ctx->device));
    Fd file;
    uint64_t file_n = 0;
    { const int rc = open_regular(ctx, path, file, &file_n); if (rc != RALA_HIP_OK) return rc; }
    // the window over the text: the overlap ingest's rule, and every count of a window in 32 bits.  A gzip file: BGZF is
    // inflated on the device, so is (option gzip_on_device) any other file of one member; what is left is the host reader's
    TextSource S;
    S.fd = file.fd;
    S.path = path;
    S.threads = threads;
    S.file_n = file_n;
    {
        bool valid = true;
        const int rc = source_open(ctx, S, ctx->gzip_on_device, nullptr, nullptr, &valid);
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
        if (trace_on()) trace_gzip(*S.gz, S.gz->windows, S.gz->window);
        if (rc == RALA_HIP_OK && !S.flag) ctx->gzip_members_last = S.gz->members;
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
            return fail(ctx, RALA_HIP_ENOMEM, "device memory for the sequence index");
        }
        SequenceColumns C;
        C.event_pos = ctx->d_seq_event[0].p; C.event_stripped = ctx->d_seq_event[1].p;
        C.name_pos = ctx->d_seq_name_pos.p; C.name_len = ctx->d_seq_name_len.p;
        C.data_off = ctx->d_seq_data_off.p; C.data_stripped = ctx->d_seq_data_stripped.p;
        HIPCHECK(hipMemsetAsync(ctx->d_seq_flags.p, 0, 4, s));
        launch_sequence_finish(R.n_records, R.n_events, R.text_n, R.n_stripped, R.fastq, C, ctx->d_seq_span.p, ctx->d_seq_length.p, ctx->d_seq_flags.p, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(&flags, ctx->d_seq_flags.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(length.data(), ctx->d_seq_length.p, R.n_records * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
    }
    kernel_ms += now_ms() - tf;
    ctx->seq_tm.ship_ms = (float)ship_ms;
    ctx->seq_tm.tokenize_ms = (float)kernel_ms;
    ctx->seq_tm.bytes = R.text_n;
    ctx->seq_tm.lines = R.n_records;
    if (trace_on()) {
        fprintf(stderr, "[trace] device sequence index: %.2f GB of text shipped in %.1f ms, %lu records indexed in %.2f ms (flags %u)\n", R.text_n / 1e9,
                ship_ms, (unsigned long)R.n_records, kernel_ms, flags);
    }
    if (flags & kSeqTooLong) return fail(ctx, RALA_HIP_ETOOLARGE, "a sequence of 2^32 bases or more");
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
    ctx->seq_gzip_members.clear();
    if (S.gz) {
        ctx->seq_gzip_chain.swap(S.gz->chain);
        ctx->seq_gzip_members.swap(S.gz->members);
        ctx->seq_gzip_crc = S.gz->crc;
    }
    *n_records = R.n_records;
    *name_bytes = R.name_bytes;
    return RALA_HIP_OK;
}

int rala_hip_get_sequence_index(rala_hip_ctx* ctx, uint64_t* name_off, uint32_t* name_len, uint64_t* data_off, uint64_t* data_span,
                                uint32_t* length, char* names) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (!ctx->seq_index_valid) return fail(ctx, RALA_HIP_EINVAL, "no sequence index (rala_hip_index_sequences)");
    HIPCHECK(hipSetDevice(ctx->device));
    const uint64_t n = ctx->n_seq_records;
    if (n && name_off) HIPCHECK(hipMemcpy(name_off, ctx->d_seq_name_off.p, n * 8, hipMemcpyDeviceToHost));
    if (n && name_len) HIPCHECK(hipMemcpy(name_len, ctx->d_seq_name_len.p, n * 4, hipMemcpyDeviceToHost));
    if (n && data_off) HIPCHECK(hipMemcpy(data_off, ctx->d_seq_data_off.p, n * 8, hipMemcpyDeviceToHost));
    if (n && data_span) HIPCHECK(hipMemcpy(data_span, ctx->d_seq_span.p, n * 8, hipMemcpyDeviceToHost));
    if (n && length) HIPCHECK(hipMemcpy(length, ctx->d_seq_length.p, n * 4, hipMemcpyDeviceToHost));
    if (ctx->n_seq_name_bytes && names) HIPCHECK(hipMemcpy(names, ctx->d_seq_arena.p, ctx->n_seq_name_bytes, hipMemcpyDeviceToHost));
    return RALA_HIP_OK;
}

int rala_hip_get_sequence_timings(rala_hip_ctx* ctx, rala_hip_ingest_timings* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->seq_tm;
    return RALA_HIP_OK;
}

int rala_hip_slice_sequences(rala_hip_ctx* ctx, const char* path, const uint64_t* wanted, uint64_t n_wanted, const uint64_t* base_off,
                             uint8_t* bases, uint32_t threads, int* irregular) {
    if (!ctx || !path || !irregular || !base_off || (n_wanted && !wanted) || (!bases && base_off[n_wanted] && !ctx->keep_bases)) return RALA_HIP_EINVAL;
    *irregular = 0;
    ctx->slice_info = rala_hip_sequence_slice_info();
    // option keep_bases: the packed bases stay on the device as the context's table of bases (spell.hip) - the windows'
    // gather writes into it, a host copy is made only where one is asked for.  Whatever was the table is gone first.
    const bool keep = ctx->keep_bases;
    if (keep) bases_released(ctx);
    if (!ctx->seq_index_valid) { *irregular = 64; return RALA_HIP_OK; }
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t n_rec = ctx->n_seq_records;
    // what the index holds of the wanted reads (none of them empty): where their text lies, where their bases go
    std::vector<uint64_t> data_off(n_rec), span(n_rec), data_stripped(n_rec);
    std::vector<uint32_t> length(n_rec);
    if (n_rec) {
        HIPCHECK(hipMemcpy(data_off.data(), ctx->d_seq_data_off.p, n_rec * 8, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(span.data(), ctx->d_seq_span.p, n_rec * 8, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(data_stripped.data(), ctx->d_seq_data_stripped.p, n_rec * 8, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(length.data(), ctx->d_seq_length.p, n_rec * 4, hipMemcpyDeviceToHost));
    }
    std::vector<uint64_t> w_off, w_end, w_adj, w_base;
    if (base_off[0] != 0) return fail(ctx, RALA_HIP_EINVAL, "base_off does not begin at 0");
    for (uint64_t k = 0; k < n_wanted; ++k) {
        const uint64_t r = wanted[k];
        if (r >= n_rec || (k && r <= wanted[k - 1])) return fail(ctx, RALA_HIP_EINVAL, "wanted reads not ascending records of the index");
        if (base_off[k + 1] - base_off[k] != length[r]) return fail(ctx, RALA_HIP_EINVAL, "base_off is not the scan of the wanted reads' lengths");
        if (!length[r]) continue;
        w_off.push_back(data_off[r]);
        w_end.push_back(data_off[r] + span[r]);
        w_adj.push_back(base_off[k] - data_off[r] + data_stripped[r]);
        w_base.push_back(base_off[k]);
    }
    const uint64_t n_w = w_off.size(), n_bases = base_off[n_wanted];
    Fd file;
    uint64_t file_n = 0;
    if (open_regular(ctx, path, file, &file_n) != RALA_HIP_OK || file_n != ctx->seq_file_n) { *irregular = 64; return RALA_HIP_OK; }
    if (!n_w) return RALA_HIP_OK;
    if (keep && ctx->d_bases.ensure(n_bases) != hipSuccess) {
        bases_released(ctx);
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for the kept bases");
    }
    // whatever way this call ends, the wanted reads, a window's bases and the source's buffers do not stay the context's
    struct Release {
        rala_hip_ctx* ctx;
        bool kept = false;                  // the table of bases was adopted: it stays
        ~Release() {
            source_close(ctx);
            ctx->d_slice_out.release();
            for (int k = 0; k < 3; ++k) ctx->d_slice_w[k].release();
            if (ctx->keep_bases && !kept) bases_released(ctx);
        }
    } release{ctx};
    for (int k = 0; k < 3; ++k) HIPCHECK(ctx->d_slice_w[k].ensure(n_w));
    HIPCHECK(hipMemcpy(ctx->d_slice_w[0].p, w_off.data(), n_w * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_slice_w[1].p, w_end.data(), n_w * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->d_slice_w[2].p, w_adj.data(), n_w * 8, hipMemcpyHostToDevice));
    TextSource S;
    S.fd = file.fd;
    S.path = path;
    S.threads = threads;
    S.file_n = file_n;
    {
        bool valid = true;
        const bool gz = ctx->seq_source == kTextGzip;
        const int rc = source_open(ctx, S, gz, gz ? &ctx->seq_gzip_chain : nullptr, gz ? &ctx->seq_gzip_members : nullptr, &valid);
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
    HIPCHECK(ctx->d_seq_flags.ensure(1));
    HIPCHECK(hipMemsetAsync(ctx->d_seq_flags.p, 0, 4, s));
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
                rc = fail(ctx, RALA_HIP_ENOMEM, "device memory for the tiles' counts");
                break;
            }
            launch_sequence_count(w.text, w.n, last_is_newline, ctx->seq_fastq, ctx->d_seq_tile[0].p, ctx->d_seq_tile[1].p, s);
            launch_exclusive_scan(ctx->d_seq_tile[1].p, ctx->d_seq_tile[1].p, n_tiles, ctx->d_scan_ws.p, s);
            uint32_t stripped = 0;
            uint8_t last = 0;
            if (hipMemcpyAsync(&stripped, ctx->d_seq_tile[1].p + n_tiles, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipMemcpyAsync(&last, w.text + w.n - 1, 1, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
                rc = fail(ctx, RALA_HIP_EDEVICE, "counting a window's stripped bytes failed");
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
                    if (!keep && ctx->d_slice_out.ensure(out_n) != hipSuccess) { rc = fail(ctx, RALA_HIP_ENOMEM, "device memory for a window's bases"); break; }
                    uint8_t* const d_out = keep ? ctx->d_bases.p + out_lo : ctx->d_slice_out.p;
                    SequenceGather G;
                    G.text = w.text; G.n = w.n; G.text_off = lo;
                    G.tile_stripped0 = ctx->d_seq_tile[1].p; G.stripped0 = n_stripped;
                    G.w_off = ctx->d_slice_w[0].p; G.w_end = ctx->d_slice_w[1].p; G.w_adj = ctx->d_slice_w[2].p;
                    G.k_lo = k_lo; G.k_hi = k_hi;
                    G.out_lo = out_lo; G.out_n = out_n; G.out = d_out; G.flags = ctx->d_seq_flags.p;
                    const double tg = now_ms();
                    launch_sequence_gather(G, s);
                    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { rc = fail(ctx, RALA_HIP_EDEVICE, "the gather kernel failed"); break; }
                    const double tc = now_ms();
                    if ((bases && hipMemcpyAsync(bases + out_lo, d_out, out_n, hipMemcpyDeviceToHost, s) != hipSuccess) ||
                        hipMemcpyAsync(&flags, ctx->d_seq_flags.p, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
                        rc = fail(ctx, RALA_HIP_EDEVICE, "copying a window's bases failed");
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
    if (trace_on()) {
        fprintf(stderr, "[trace] device sequence slice: %lu windows of at most %.3f GB of text, %lu bases of %lu reads, ship %.1f ms, device %.2f ms "
                "(gather %.2f ms, bases to the host %.2f ms) (flags %u)\n", (unsigned long)S.windows, S.max_window / 1e9,
                (unsigned long)ctx->slice_info.bases, (unsigned long)n_wanted, S.ship_ms, kernel_ms, gather_ms, copy_ms, S.flag | flags);
    }
    if (S.flag || flags) *irregular = (int)(S.flag | flags);
    if (keep && !*irregular) {
        const int rck = bases_adopted(ctx, base_off, n_wanted, true);
        if (rck != RALA_HIP_OK) return rck;
        release.kept = true;
    }
    return RALA_HIP_OK;
}

int rala_hip_get_sequence_slice_info(rala_hip_ctx* ctx, rala_hip_sequence_slice_info* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->slice_info;
    return RALA_HIP_OK;
}

}  // extern "C"
