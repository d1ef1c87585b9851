// A gzip file that is not BGZF (gzip, pigz, Python's gzip; with the option gzip_members any chain of such members: cat a.gz b.gz,
// pigz -i) inflated on the device by speculative decoding (inflate_kernels.hip).
// One front half - the file shipped, member headers and block starts found, every chunk and every member candidate counted from
// its start, the chain from chunk 0 built and proven on the host - and two back ends: the whole text at once (overlap files)
// or window by window (read files).  Either proves every member: its ISIZE in the chain, its CRC32 from the registers of the
// 16 KB segments that lie inside it and of the pieces of those a member boundary cuts.
// A third way for one member and the ranks of a sharded run (option gzip_in_pieces): every rank its own chunks of the stream, in
// steps with the ranks' exchanges between them (gzip_piece_*, below).
#include "ingest_common.h"

using namespace rala_hip;
using namespace rala_hip::ingest;

namespace {

// The member headers among the n bytes at comp (launch_gzip_member_count / _write): counted per tile, scanned, written - to
// ctx->d_gzip_cands, *n_cands of them in ascending order.
int gzip_member_find(rala_hip_ctx* ctx, const uint8_t* comp, uint64_t n, uint64_t* n_cands) {
    hipStream_t s = ctx->stream;
    *n_cands = 0;
    const uint64_t n_tiles = (n + gzip_member_tile_bytes() - 1) / gzip_member_tile_bytes();
    if (!n_tiles) return RALA_HIP_OK;
    if (n_tiles >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "file too large for 32-bit tile ids");
    if (ctx->d_gzip_tile.ensure(n_tiles + 2) != hipSuccess || ctx->d_scan_ws.ensure(scan_workspace_bytes(n_tiles + 2)) != hipSuccess) {
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for the member find");
    }
    launch_gzip_member_count(comp, n, ctx->d_gzip_tile.p, s);
    launch_exclusive_scan(ctx->d_gzip_tile.p, ctx->d_gzip_tile.p, n_tiles, ctx->d_scan_ws.p, s);
    HIPCHECK(hipGetLastError());
    uint32_t total = 0;
    HIPCHECK(hipMemcpyAsync(&total, ctx->d_gzip_tile.p + n_tiles, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (ctx->d_gzip_cands.ensure(((size_t)total + 1) * sizeof(GzipMemberCand)) != hipSuccess) {
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for the member find");
    }
    launch_gzip_member_write(comp, n, ctx->d_gzip_tile.p, (GzipMemberCand*)ctx->d_gzip_cands.p, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    *n_cands = total;
    return RALA_HIP_OK;
}

// where the text of every job's member begins
void job_floors(GzipStream& g) {
    g.job_floor.resize(g.chain.size());
    size_t m = 0;
    for (size_t j = 0; j < g.chain.size(); ++j) {
        if (j && g.chain[j].first && m + 1 < g.members.size()) ++m;
        g.job_floor[j] = g.members[m].text_off;
    }
}

// The file (g.file_n bytes) to ctx->d_bgzf_comp, where it stays, and its chain: found / counted on the device and built by
// gzip_chain_from_spans (option gzip_members: gzip_chain_members), or (given != null) the chain and the members of an earlier
// call taken over.  *valid = false: not a stream this can prove - a header the parse refuses, what the chain builder refuses,
// a chain taken over that is not this file's (a member's ISIZE or CRC32 is no longer the one it was taken with).
int gzip_chain_open(rala_hip_ctx* ctx, int fd, const char* path, uint32_t threads, const std::vector<GzipJob>* given,
                    const std::vector<GzipMember>* given_members, GzipStream& g, bool* valid) {
    *valid = false;
    const uint64_t file_n = g.file_n;
    std::vector<uint8_t> head((size_t)std::min(file_n, kGzipHeadReach));
    uint8_t trailer[8];
    if (file_n < 18 || pread(fd, head.data(), head.size(), 0) != (ssize_t)head.size() || pread(fd, trailer, 8, (off_t)(file_n - 8)) != 8) return RALA_HIP_OK;
    uint64_t deflate_off = 0;
    if (!gzip_head(head.data(), head.size(), &deflate_off) || deflate_off + 8 >= file_n) return RALA_HIP_OK;
    const uint64_t end = g.end = file_n - 8;
    g.crc = le32(trailer);
    const uint64_t chunk = (uint64_t)std::max<int64_t>(1024, ctx->gzip_chunk_bytes);
    const uint64_t n_chunks = (end - deflate_off + chunk - 1) / chunk;
    if (!given && n_chunks >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "file too large for 32-bit chunk ids");
    hipStream_t s = ctx->stream;
    const double t0 = now_ms();
    if (ctx->d_bgzf_comp.ensure(file_n + 64) != hipSuccess || ctx->d_bgzf_flag.ensure(1) != hipSuccess) {
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
    }
    const uint8_t* comp = ctx->d_bgzf_comp.p;
    HIPCHECK(hipMemsetAsync(ctx->d_bgzf_comp.p + file_n, 0, 64, s));
    HIPCHECK(hipMemsetAsync(ctx->d_bgzf_flag.p, 0, 4, s));
    if (ship_file(fd, 0, file_n, ctx->d_bgzf_comp.p, ctx->device, threads, nullptr, []() { return true; }, &g.n_readers)) {
        return fail(ctx, RALA_HIP_EDEVICE, std::string("reading / copying ") + path + " failed");
    }
    HIPCHECK(hipStreamSynchronize(s));
    const double t1 = now_ms();
    g.ship_ms = (float)(t1 - t0);
    rala_hip_gzip_timings& tm = g.tm;
    tm.compressed_bytes = file_n;
    if (given) {
        g.chain = *given;
        if (given_members) g.members = *given_members;
        if (g.chain.empty() || g.members.empty()) return RALA_HIP_OK;
        for (const GzipJob& j : g.chain) {
            g.text_n += j.text_n;
            tm.max_wave_text_bytes = std::max<uint64_t>(tm.max_wave_text_bytes, j.text_n);
        }
        tm.chunks_confirmed = g.chain.size() - g.members.size();
        tm.text_bytes = g.text_n;
        // every member's trailer is still where it was and says what it said
        bool same = g.members.back().trailer_off + 8 == file_n;
        for (size_t m = 0; same && m < g.members.size(); ++m) {
            const GzipMember& mem = g.members[m];
            uint8_t t[8];
            same = mem.trailer_off + 8 <= file_n && pread(fd, t, 8, (off_t)mem.trailer_off) == 8 && le32(t) == mem.crc && le32(t + 4) == (uint32_t)mem.text_n;
        }
        job_floors(g);
        *valid = same;
        return RALA_HIP_OK;
    }
    const bool members = ctx->gzip_members;
    uint64_t n_cands = 0;
    if (members) {
        const int rc = gzip_member_find(ctx, comp, file_n, &n_cands);
        if (rc != RALA_HIP_OK) return rc;
        if (n_chunks + n_cands >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "too many member candidates for 32-bit span ids");
    }
    const double t1b = now_ms();
    g.n_cands = n_cands;
    g.member_find_ms = (float)(t1b - t1);
    if (ctx->d_gzip_starts.ensure(n_chunks) != hipSuccess || ctx->d_gzip_spans.ensure(n_chunks * sizeof(GzipSpan)) != hipSuccess ||
        ctx->d_gzip_mspans.ensure((n_cands + 1) * sizeof(GzipSpan)) != hipSuccess) {
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
    }
    launch_gzip_find(comp, end, (file_n + 56) / 8, deflate_off, chunk, (uint32_t)n_chunks, ctx->debug_gzip_false_sync, ctx->d_gzip_starts.p, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    const double t2 = now_ms();
    launch_gzip_count(comp, end, ctx->d_gzip_starts.p, (uint32_t)n_chunks, (GzipSpan*)ctx->d_gzip_spans.p, s, (const GzipMemberCand*)ctx->d_gzip_cands.p,
                      (uint32_t)n_cands, deflate_off, chunk, (GzipSpan*)ctx->d_gzip_mspans.p);
    HIPCHECK(hipGetLastError());
    std::vector<uint64_t> starts(n_chunks);
    std::vector<GzipSpan> spans(n_chunks), mspans(n_cands);
    std::vector<GzipMemberCand> cands(n_cands);
    HIPCHECK(hipMemcpyAsync(starts.data(), ctx->d_gzip_starts.p, n_chunks * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(spans.data(), ctx->d_gzip_spans.p, n_chunks * sizeof(GzipSpan), hipMemcpyDeviceToHost, s));
    if (n_cands) {
        HIPCHECK(hipMemcpyAsync(cands.data(), ctx->d_gzip_cands.p, n_cands * sizeof(GzipMemberCand), hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(mspans.data(), ctx->d_gzip_mspans.p, n_cands * sizeof(GzipSpan), hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    const double t3 = now_ms();
    ctx->d_gzip_starts.release();
    ctx->d_gzip_spans.release();
    ctx->d_gzip_mspans.release();
    ctx->d_gzip_cands.release();
    ctx->d_gzip_tile.release();
    tm.chunks = n_chunks;
    tm.find_ms = (float)(t2 - t1);                          // (the member find included)
    tm.decode_ms = (float)(t3 - t2);
    if (members) {
        *valid = gzip_chain_members(starts.data(), spans.data(), n_chunks, cands.data(), mspans.data(), n_cands, file_n, le32(trailer), le32(trailer + 4),
                                    g.chain, g.members, &tm);
    } else {
        *valid = gzip_chain_from_spans(starts.data(), spans.data(), n_chunks, end, le32(trailer + 4), g.chain, &tm);
        g.members.assign(1, GzipMember{0, tm.text_bytes, end, g.crc, 0});
    }
    g.text_n = tm.text_bytes;
    if (*valid) job_floors(g);
    return RALA_HIP_OK;
}

// The members' CRC32 behind a launch that left the text [lo, lo + n) at `text` and its segments' registers in seg_crc: the
// members from g.proven on take the registers of the segments that lie inside them and those of the pieces a member boundary
// cuts off a segment (gzip_piece_crc_kernel: at most two per boundary, one per member that lies inside one segment); a member
// that ends here is compared with its trailer, one that goes on keeps one register for the next launch.
int gzip_prove_members(rala_hip_ctx* ctx, GzipStream& g, const uint8_t* text, uint64_t lo, uint64_t n, const std::vector<uint32_t>& seg_crc) {
    hipStream_t s = ctx->stream;
    const uint64_t seg = gzip_segment_bytes();
    struct Item { uint64_t idx, len; int kind; };                    // kind 0: segment idx, 1: piece idx, 2: the member ends
    std::vector<Item> items;
    std::vector<GzipPiece> pieces;
    for (size_t m = g.proven; m < g.members.size(); ++m) {
        const GzipMember& mem = g.members[m];
        const uint64_t m_end = mem.text_off + mem.text_n, hi = std::min(m_end, lo + n);
        for (uint64_t p = std::max(mem.text_off, lo); p < hi;) {
            const uint64_t k = (p - lo) / seg, seg_lo = lo + k * seg, seg_hi = std::min(seg_lo + seg, lo + n), q = std::min(hi, seg_hi);
            if (p == seg_lo && q == seg_hi) {
                items.push_back(Item{k, q - p, 0});
            } else {
                items.push_back(Item{pieces.size(), q - p, 1});
                pieces.push_back(GzipPiece{p - lo, (uint32_t)(q - p), 0});
            }
            p = q;
        }
        if (m_end > lo + n) break;
        items.push_back(Item{m, 0, 2});
    }
    std::vector<uint32_t> piece_crc(pieces.size());
    if (!pieces.empty()) {
        if (pieces.size() >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "too many member boundaries in one window");
        if (ctx->d_gzip_pieces.ensure(pieces.size() * sizeof(GzipPiece)) != hipSuccess || ctx->d_gzip_piece_crc.ensure(pieces.size()) != hipSuccess) {
            return fail(ctx, RALA_HIP_ENOMEM, "device memory for the members' pieces");
        }
        HIPCHECK(hipMemcpyAsync(ctx->d_gzip_pieces.p, pieces.data(), pieces.size() * sizeof(GzipPiece), hipMemcpyHostToDevice, s));
        launch_gzip_piece_crc(text, (const GzipPiece*)ctx->d_gzip_pieces.p, (uint32_t)pieces.size(), ctx->d_gzip_piece_crc.p, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(piece_crc.data(), ctx->d_gzip_piece_crc.p, pieces.size() * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
    }
    for (const Item& it : items) {
        if (it.kind == 2) {
            if (gzip_crc_chain(g.reg.data(), g.len.data(), g.reg.size()) != g.members[it.idx].crc) g.crc_ok = false;
            g.reg.clear();
            g.len.clear();
            g.proven = it.idx + 1;
        } else {
            g.reg.push_back(it.kind ? piece_crc[it.idx] : seg_crc[it.idx]);
            g.len.push_back(it.len);
        }
    }
    if (g.reg.size() > 1) {
        uint64_t total = 0;
        for (uint64_t l : g.len) total += l;
        const uint32_t r = gzip_crc_register_chain(g.reg.data(), g.len.data(), g.reg.size());
        g.reg.assign(1, r);
        g.len.assign(1, total);
    }
    return RALA_HIP_OK;
}

}  // namespace

// Written and resolved in one piece behind the front half (no window, so no 2^31 cap on the text), every member's CRC32 checked.
int rala_hip::ingest::gzip_inflate(rala_hip_ctx* ctx, int fd, const char* path, uint32_t threads, GzipStream& g, bool* valid) {
    const int rc = gzip_chain_open(ctx, fd, path, threads, nullptr, nullptr, g, valid);
    if (rc != RALA_HIP_OK || !*valid) return rc;
    *valid = false;
    hipStream_t s = ctx->stream;
    const uint64_t text_n = g.text_n, n_jobs = g.chain.size();
    std::vector<uint64_t> text_off(n_jobs);
    for (size_t j = 0; j < n_jobs; ++j) text_off[j] = g.chain[j].text_off;
    const uint64_t n_seg = (text_n + gzip_segment_bytes() - 1) / gzip_segment_bytes();
    if (n_seg >= 0xFFFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "text too large for 32-bit segment ids");
    if (ctx->d_gzip_sym.ensure(text_n + 64) != hipSuccess || ctx->d_gzip_text.ensure(text_n + paf_chunk_bytes() + 8192) != hipSuccess ||
        ctx->d_gzip_jobs.ensure(n_jobs * sizeof(GzipJob)) != hipSuccess || ctx->d_gzip_off.ensure(n_jobs) != hipSuccess ||
        ctx->d_gzip_floor.ensure(n_jobs) != hipSuccess || ctx->d_gzip_crc.ensure(n_seg + 1) != hipSuccess) {
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for the inflated text");
    }
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_jobs.p, g.chain.data(), n_jobs * sizeof(GzipJob), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_off.p, text_off.data(), n_jobs * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_floor.p, g.job_floor.data(), n_jobs * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));
    const double t3 = now_ms();
    launch_gzip_write(ctx->d_bgzf_comp.p, g.end, (const GzipJob*)ctx->d_gzip_jobs.p, (uint32_t)n_jobs, ctx->d_gzip_sym.p, ctx->d_bgzf_flag.p, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    const double t4 = now_ms();
    launch_gzip_resolve(ctx->d_gzip_sym.p, ctx->d_gzip_off.p, ctx->d_gzip_floor.p, (uint32_t)n_jobs, text_n, ctx->d_gzip_text.p, ctx->d_gzip_crc.p,
                        ctx->d_bgzf_flag.p, s);
    HIPCHECK(hipGetLastError());
    // what lies behind the text reads as newlines (as for the plain file)
    HIPCHECK(hipMemsetAsync(ctx->d_gzip_text.p + text_n, '\n', paf_chunk_bytes() + 8192, s));
    std::vector<uint32_t> seg_crc(n_seg);
    uint32_t flag = 0;
    if (n_seg) HIPCHECK(hipMemcpyAsync(seg_crc.data(), ctx->d_gzip_crc.p, n_seg * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(&flag, ctx->d_bgzf_flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (!flag) { const int rcp = gzip_prove_members(ctx, g, ctx->d_gzip_text.p, 0, text_n, seg_crc); if (rcp != RALA_HIP_OK) return rcp; }
    const double t5 = now_ms();
    ctx->d_gzip_sym.release();
    ctx->d_bgzf_comp.release();
    g.tm.decode_ms += (float)(t4 - t3);                     // the counting pass and the writing pass
    g.tm.resolve_ms = (float)(t5 - t4);
    *valid = !flag && g.crc_ok && g.proven == g.members.size();
    return RALA_HIP_OK;
}

// ---- WINDOW by window (the driver of the same kernels for a text that does not fit): the compressed file stays resident -
// the only buffer whose size depends on the file's; write, windows and resolve run per window, a run of consecutive true
// chunks whose text fits it.  The symbols of a window lie behind a CARRY of gzip_ring_symbols(): the last 32 768 bytes in
// front of it (0x8000 where the file's text has not begun), so the markers of its first chunks point into bytes, and every
// text offset the kernels see counts from the carry's first symbol.  A window may hold any number of member boundaries: a
// member's first chunk emits no markers, so the carry needs no reset, and a marker of a later chunk that reaches below its
// member's first byte - in the carry or not - is refused by the floor the kernels get beside every text offset.
// The front half (chain != null: the chain and the members of an earlier walk taken over), then the buffers of a window made:
// `front` bytes of room in front of the window's text in ctx->d_gzip_text and `behind` bytes behind it.  want_window 0: what a
// quarter of the free memory holds at three bytes per text byte.  *valid = false: not a stream this can prove.
int rala_hip::ingest::gzip_walk_open(rala_hip_ctx* ctx, int fd, const char* path, uint32_t threads, uint64_t want_window, uint64_t front,
                                     uint64_t behind, const std::vector<GzipJob>* chain, const std::vector<GzipMember>* members, GzipWalk& g,
                                     bool* valid) {
    const int rc = gzip_chain_open(ctx, fd, path, threads, chain, members, g, valid);
    if (rc != RALA_HIP_OK || !*valid) return rc;
    *valid = false;
    hipStream_t s = ctx->stream;
    // the window: symbols (2 bytes) and text (1 byte) of it inside the quarter of what is free now
    uint64_t window = want_window;
    if (window == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        window = std::max<uint64_t>(64ull << 20, free_b / 12);
    }
    window = std::max<uint64_t>(std::min<uint64_t>(window, 1ull << 31), g.tm.max_wave_text_bytes);
    if (window > (1ull << 31)) return fail(ctx, RALA_HIP_ENOMEM, "a chunk of the gzip file gives more text than a window holds");
    window = std::min(window, std::max<uint64_t>(g.text_n, 1));
    g.window = window;
    const uint64_t ring = gzip_ring_symbols();
    if (ctx->d_gzip_sym.ensure(ring + window + 64) != hipSuccess || ctx->d_gzip_text.ensure(front + window + behind) != hipSuccess ||
        ctx->d_gzip_crc.ensure(window / gzip_segment_bytes() + 2) != hipSuccess || ctx->d_gzip_carry.ensure(ring) != hipSuccess ||
        ctx->d_gzip_hold.ensure(front + 16) != hipSuccess) {
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for a window of the inflated text");
    }
    // nothing lies in front of the first window: a marker that points there is no byte
    HIPCHECK(hipMemsetD16Async((hipDeviceptr_t)ctx->d_gzip_sym.p, (unsigned short)0x8000u, ring, s));
    *valid = true;
    return RALA_HIP_OK;
}

// The next window's text [*lo, *lo + *n) to `text` (16-byte aligned, in ctx->d_gzip_text).  *flag != 0: the inflater refused.
int rala_hip::ingest::gzip_walk_next(rala_hip_ctx* ctx, GzipWalk& g, uint8_t* text, uint64_t* lo, uint64_t* n, uint32_t* flag) {
    hipStream_t s = ctx->stream;
    const uint64_t ring = gzip_ring_symbols();
    const size_t j0 = g.next_job;
    size_t j1 = j0;
    uint64_t n_w = 0;
    while (j1 < g.chain.size() && (j1 == j0 || n_w + g.chain[j1].text_n <= g.window)) n_w += g.chain[j1++].text_n;
    const uint64_t a = g.chain[j0].text_off;
    std::vector<GzipJob> jobs(g.chain.begin() + j0, g.chain.begin() + j1);
    std::vector<uint64_t> text_off(jobs.size()), floors(jobs.size());
    for (size_t j = 0; j < jobs.size(); ++j) {
        text_off[j] = jobs[j].text_off = ring + (jobs[j].text_off - a);
        // the member's first text position in this launch's coordinates, the carry's first symbol at the least
        const uint64_t f = g.job_floor[j0 + j];
        floors[j] = f + ring >= a ? f + ring - a : 0;
    }
    if (n_w > g.window) return fail(ctx, RALA_HIP_EDEVICE, "a chunk larger than the window");
    *lo = a;
    *n = n_w;
    *flag = 0;
    g.next_job = j1;
    if (ctx->d_gzip_jobs.ensure(jobs.size() * sizeof(GzipJob)) != hipSuccess || ctx->d_gzip_off.ensure(jobs.size()) != hipSuccess ||
        ctx->d_gzip_floor.ensure(jobs.size()) != hipSuccess) {
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for a window's chunks");
    }
    const double t0 = now_ms();
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_jobs.p, jobs.data(), jobs.size() * sizeof(GzipJob), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_off.p, text_off.data(), text_off.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_floor.p, floors.data(), floors.size() * 8, hipMemcpyHostToDevice, s));
    launch_gzip_write(ctx->d_bgzf_comp.p, g.end, (const GzipJob*)ctx->d_gzip_jobs.p, (uint32_t)jobs.size(), ctx->d_gzip_sym.p, ctx->d_bgzf_flag.p, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    const double t1 = now_ms();
    const uint64_t n_seg = (n_w + gzip_segment_bytes() - 1) / gzip_segment_bytes();
    launch_gzip_resolve(ctx->d_gzip_sym.p, ctx->d_gzip_off.p, ctx->d_gzip_floor.p, (uint32_t)jobs.size(), n_w, text, ctx->d_gzip_crc.p, ctx->d_bgzf_flag.p,
                        s, ring);
    HIPCHECK(hipGetLastError());
    std::vector<uint32_t> seg_crc(n_seg);
    if (n_seg) HIPCHECK(hipMemcpyAsync(seg_crc.data(), ctx->d_gzip_crc.p, n_seg * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(flag, ctx->d_bgzf_flag.p, 4, hipMemcpyDeviceToHost, s));
    if (j1 < g.chain.size()) launch_gzip_carry(ctx->d_gzip_sym.p, text, n_w, ctx->d_gzip_carry.p, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    if (!*flag) { const int rc = gzip_prove_members(ctx, g, text, a, n_w, seg_crc); if (rc != RALA_HIP_OK) return rc; }
    g.tm.decode_ms += (float)(t1 - t0);
    g.tm.resolve_ms += (float)(now_ms() - t1);
    ++g.windows;
    return RALA_HIP_OK;
}

// behind the last window: was every member's text its trailer's?
bool rala_hip::ingest::gzip_walk_proven(const GzipWalk& g) {
    return g.next_job == g.chain.size() && g.proven == g.members.size() && g.crc_ok;
}

// ---- in PIECES over the ranks of a sharded run (option gzip_in_pieces; the collectives between the steps: sharded.hip) --------
// The writing pass gives symbols that name the 32 768 bytes in front of a chunk without knowing them, so a rank decodes its own
// chunks of the stream without a byte of the text in front of them; what travels is every chunk's start and span (so that every
// rank builds the same chain) and one window of 32 768 symbols per rank (so that every rank learns the bytes in front of its
// piece).  Every rank ships the whole compressed file; windows inside a piece are not made: own text and halo fit at once or
// the step fails with ENOMEM.
struct rala_hip::GzipPieceRun {
    Fd file;
    std::string path;
    uint64_t file_n = 0, deflate_off = 0, end = 0, chunk = 0, n_chunks = 0;
    uint32_t crc = 0, isize = 0;
    uint32_t part = 0, parts = 1;
    uint64_t c0 = 0, c1 = 0, most = 0;          // own chunks; the most chunks any part owns
    std::vector<uint64_t> starts;               // of all chunks, behind the first exchange
    std::vector<GzipJob> chain;                 // the same on every rank
    size_t j0 = 0, j1 = 0, j2 = 0;              // own jobs [j0, j1), written jobs [j0, j2)
    uint64_t a = 0, b = 0, n_w = 0;             // own text [a, b), written text [a, a + n_w)
    uint32_t n_readers = 0;
    float ship_ms = 0;
    rala_hip_gzip_timings tm = {};
    rala_hip_gzip_pieces_info info = {};
    // a file of several members (option gzip_members): the header candidates of the whole file and the part each one's deflate
    // bytes begin in (the same on every rank), the most any part owns; behind the chain the members, every job's member floor
    // and every part's first job
    bool members_mode = false, cands_agree = true, cands_split = false;
    std::vector<GzipMemberCand> cands;
    std::vector<uint32_t> cand_part;
    uint64_t most_cands = 0;
    std::vector<GzipMember> members;
    std::vector<uint64_t> job_floor, first_job;
    float member_find_ms = 0;
    rala_hip_gzip_member_pieces_info minfo = {};
};

namespace {
// the part whose chunks hold the byte a candidate's deflate bytes begin at (the chunk gzip_count_members_kernel starts from)
uint32_t part_of_bit(const GzipPieceRun* g, uint64_t bit) {
    const uint64_t byte = bit / 8, c = std::min((byte - std::min(byte, g->deflate_off)) / g->chunk, g->n_chunks - 1);
    uint32_t p = 0;
    while (p + 1 < g->parts && c >= gzip_part_chunk(g->n_chunks, g->parts, p + 1)) ++p;
    return p;
}
}  // namespace

namespace {
// Behind the resolve of a piece of a file of several members: the text [a, a + n_w) at `text`, its segments' registers in seg_crc.
// Every member's share of the own text [a, b) gets its register - whole segments', and gzip_piece_crc_kernel's for the pieces a
// member end or b cuts off a segment; a member that lies inside [a, b) is compared with its trailer here (own[6]: the first one
// that differs), the head and the tail the piece owes members that span ranks go to own[2 .. 5].
int piece_prove_members(rala_hip_ctx* ctx, GzipPieceRun* g, const uint8_t* text, const std::vector<uint32_t>& seg_crc, uint64_t own[7]) {
    hipStream_t s = ctx->stream;
    const uint64_t seg = gzip_segment_bytes(), a = g->a, b = g->b, n_w = g->n_w;
    struct Item { uint64_t idx, len; bool piece; };
    struct Share { size_t m, first, n; int kind; };                  // kind 0: inside, 1: head, 2: tail
    std::vector<Item> items;
    std::vector<Share> shares;
    std::vector<GzipPiece> pieces;
    for (size_t m = 0; m < g->members.size(); ++m) {
        const GzipMember& mem = g->members[m];
        const uint64_t m_end = mem.text_off + mem.text_n, lo = std::max(mem.text_off, a), hi = std::min(m_end, b);
        if (lo >= hi) continue;
        Share sh{m, items.size(), 0, mem.text_off < a ? 1 : (m_end > b ? 2 : 0)};
        for (uint64_t p = lo; p < hi;) {
            const uint64_t k = (p - a) / seg, seg_lo = a + k * seg, seg_hi = std::min(seg_lo + seg, a + n_w), q = std::min(hi, seg_hi);
            if (p == seg_lo && q == seg_hi) {
                items.push_back(Item{k, q - p, false});
            } else {
                items.push_back(Item{pieces.size(), q - p, true});
                pieces.push_back(GzipPiece{p - a, (uint32_t)(q - p), 0});
            }
            p = q;
        }
        sh.n = items.size() - sh.first;
        shares.push_back(sh);
    }
    std::vector<uint32_t> piece_crc(pieces.size());
    if (!pieces.empty()) {
        if (pieces.size() >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "too many member boundaries in one piece");
        if (ctx->d_gzip_pieces.ensure(pieces.size() * sizeof(GzipPiece)) != hipSuccess || ctx->d_gzip_piece_crc.ensure(pieces.size()) != hipSuccess) {
            return fail(ctx, RALA_HIP_ENOMEM, "device memory for the members' pieces");
        }
        HIPCHECK(hipMemcpyAsync(ctx->d_gzip_pieces.p, pieces.data(), pieces.size() * sizeof(GzipPiece), hipMemcpyHostToDevice, s));
        launch_gzip_piece_crc(text, (const GzipPiece*)ctx->d_gzip_pieces.p, (uint32_t)pieces.size(), ctx->d_gzip_piece_crc.p, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(piece_crc.data(), ctx->d_gzip_piece_crc.p, pieces.size() * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
    }
    for (const Share& sh : shares) {
        std::vector<uint32_t> reg(sh.n);
        std::vector<uint64_t> len(sh.n);
        uint64_t total = 0;
        for (size_t i = 0; i < sh.n; ++i) {
            const Item& it = items[sh.first + i];
            reg[i] = it.piece ? piece_crc[it.idx] : seg_crc[it.idx];
            total += len[i] = it.len;
        }
        if (sh.kind == 0) {
            if (gzip_crc_chain(reg.data(), len.data(), sh.n) != g->members[sh.m].crc && own[6] == ~0ull) own[6] = sh.m;
        } else {
            own[sh.kind == 1 ? 2 : 4] = gzip_crc_register_chain(reg.data(), len.data(), sh.n);
            own[sh.kind == 1 ? 3 : 5] = total;
            ++g->minfo.registers_sent;
        }
    }
    return RALA_HIP_OK;
}
}  // namespace

uint64_t rala_hip::gzip_piece_most_chunks(uint64_t n_chunks, uint32_t parts) {
    uint64_t most = 0;
    for (uint32_t k = 0; k < parts; ++k) most = std::max(most, gzip_part_chunk(n_chunks, parts, k + 1) - gzip_part_chunk(n_chunks, parts, k));
    return most;
}

int rala_hip::gzip_piece_open(rala_hip_ctx* ctx, const char* path, bool mhap, uint64_t head[7], GzipPieceRun** run) {
    for (int k = 0; k < 7; ++k) head[k] = 0;
    head[6] = ctx->gzip_members ? 1 : 0;
    *run = nullptr;
    std::unique_ptr<GzipPieceRun> g(new GzipPieceRun());
    g->path = path;
    g->members_mode = ctx->gzip_members;
    ctx->gzip_pieces = rala_hip_gzip_pieces_info();
    ctx->gzip_member_pieces = rala_hip_gzip_member_pieces_info();
    if (g->members_mode) ctx->gzip_members_last.clear();
    int rc = ingest_ready(ctx, mhap);
    if (rc != RALA_HIP_OK) return rc;
    rc = open_regular(ctx, path, g->file, &g->file_n);
    if (rc != RALA_HIP_OK) return rc;
    const uint64_t file_n = g->file_n;
    std::vector<uint8_t> first((size_t)std::min(file_n, kGzipHeadReach));
    uint8_t trailer[8];
    if (file_n >= 18 && pread(g->file.fd, first.data(), first.size(), 0) == (ssize_t)first.size() && pread(g->file.fd, trailer, 8, (off_t)(file_n - 8)) == 8 &&
        sniff(first.data(), first.size()) == kTextGzip && gzip_head(first.data(), first.size(), &g->deflate_off) && g->deflate_off + 8 < file_n) {
        g->end = file_n - 8;
        g->crc = le32(trailer);
        g->isize = le32(trailer + 4);
        g->chunk = (uint64_t)std::max<int64_t>(1024, ctx->gzip_chunk_bytes);
        g->n_chunks = (g->end - g->deflate_off + g->chunk - 1) / g->chunk;
        if (g->n_chunks >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "file too large for 32-bit chunk ids");
        head[0] = 1; head[1] = file_n; head[2] = g->deflate_off; head[3] = g->n_chunks;
        head[4] = g->crc; head[5] = g->isize;
    }
    *run = g.release();
    return RALA_HIP_OK;
}

void rala_hip::gzip_piece_close(rala_hip_ctx* ctx, GzipPieceRun* run) {
    if (!run) return;
    ctx->d_bgzf_comp.release();
    ctx->d_gzip_sym.release();
    ctx->d_gzip_text.release();
    ctx->d_gzip_starts.release();
    ctx->d_gzip_spans.release();
    ctx->d_gzip_carry.release();
    ctx->d_gzip_compose_stats.release();
    ctx->d_gzip_cands.release();
    ctx->d_gzip_mspans.release();
    ctx->d_gzip_tile.release();
    delete run;
}

// a. the file shipped, block starts found in the own chunks -> starts_out: `most` + 1 words, the own chunks' first, the last one
// the member headers found in the whole file (option gzip_members; otherwise 0)
int rala_hip::gzip_piece_find(rala_hip_ctx* ctx, GzipPieceRun* g, uint32_t part, uint32_t parts, uint32_t threads, std::vector<uint64_t>& starts_out) {
    g->part = part;
    g->parts = parts;
    g->c0 = gzip_part_chunk(g->n_chunks, parts, part);
    g->c1 = gzip_part_chunk(g->n_chunks, parts, part + 1);
    g->most = gzip_piece_most_chunks(g->n_chunks, parts);
    starts_out.assign(g->most + 1, kGzipNoStart);
    starts_out[g->most] = 0;
    hipStream_t s = ctx->stream;
    const uint64_t file_n = g->file_n;
    const double t0 = now_ms();
    if (ctx->d_bgzf_comp.ensure(file_n + 64) != hipSuccess || ctx->d_bgzf_flag.ensure(1) != hipSuccess || ctx->d_gzip_starts.ensure(g->n_chunks) != hipSuccess ||
        ctx->d_gzip_spans.ensure(g->n_chunks * sizeof(GzipSpan)) != hipSuccess) {
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
    }
    HIPCHECK(hipMemsetAsync(ctx->d_bgzf_comp.p + file_n, 0, 64, s));
    HIPCHECK(hipMemsetAsync(ctx->d_bgzf_flag.p, 0, 4, s));
    if (ship_file(g->file.fd, 0, file_n, ctx->d_bgzf_comp.p, ctx->device, threads, nullptr, []() { return true; }, &g->n_readers)) {
        return fail(ctx, RALA_HIP_EDEVICE, "reading / copying " + g->path + " failed");
    }
    HIPCHECK(hipStreamSynchronize(s));
    const double t1 = now_ms();
    g->ship_ms = (float)(t1 - t0);
    g->tm.compressed_bytes = file_n;
    g->tm.chunks = g->n_chunks;
    launch_gzip_find_range(ctx->d_bgzf_comp.p, g->end, (file_n + 56) / 8, g->deflate_off, g->chunk, (uint32_t)g->c0, (uint32_t)g->c1, ctx->debug_gzip_false_sync,
                           ctx->d_gzip_starts.p, s);
    HIPCHECK(hipGetLastError());
    if (g->c1 > g->c0) HIPCHECK(hipMemcpyAsync(starts_out.data(), ctx->d_gzip_starts.p + g->c0, (g->c1 - g->c0) * 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (g->members_mode) {
        // every rank over the whole file: the list is exact and ascending, the same everywhere without an exchange
        const double tm0 = now_ms();
        uint64_t n_cands = 0;
        const int rc = gzip_member_find(ctx, ctx->d_bgzf_comp.p, file_n, &n_cands);
        if (rc != RALA_HIP_OK) return rc;
        if (g->n_chunks + n_cands >= 0x7FFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "too many member candidates for 32-bit span ids");
        g->cands.resize(n_cands);
        if (n_cands) HIPCHECK(hipMemcpy(g->cands.data(), ctx->d_gzip_cands.p, n_cands * sizeof(GzipMemberCand), hipMemcpyDeviceToHost));
        ctx->d_gzip_tile.release();
        starts_out[g->most] = n_cands;
        g->member_find_ms = (float)(now_ms() - tm0);
    }
    g->tm.find_ms = (float)(now_ms() - t1);
    g->info.own_chunks = g->c1 - g->c0;
    return RALA_HIP_OK;
}

// b. all: every part's `most` start words at all[p * stride + 1 ..]; the own chunks counted, each landing on the starts behind it
// wherever they were found -> spans_out: 4 words per chunk {end_bit, text, next | status << 32, refuted}; behind the `most` chunks
// (option gzip_members) 4 words per member candidate whose deflate bytes begin in the own chunks, decoded from its first block as
// from a stream's first chunk, padded to the most candidates any part owns (gzip_piece_span_words)
int rala_hip::gzip_piece_count(rala_hip_ctx* ctx, GzipPieceRun* g, const uint64_t* all, size_t stride, std::vector<uint64_t>& spans_out) {
    hipStream_t s = ctx->stream;
    spans_out.assign(gzip_piece_span_words(g, all, stride), 0);
    g->starts.assign(g->n_chunks, kGzipNoStart);
    for (uint32_t p = 0; p < g->parts; ++p) {
        const uint64_t lo = gzip_part_chunk(g->n_chunks, g->parts, p), hi = gzip_part_chunk(g->n_chunks, g->parts, p + 1);
        for (uint64_t c = lo; c < hi; ++c) g->starts[c] = all[(size_t)p * stride + 1 + (c - lo)];
    }
    const double t0 = now_ms();
    std::vector<GzipSpan> mspans;
    if (g->members_mode && g->cands_agree) {
        // the own candidates, against the starts as they are (the launch below blinds one of them)
        std::vector<GzipMemberCand> own;
        for (size_t k = 0; k < g->cands.size(); ++k) if (g->cand_part[k] == g->part) own.push_back(g->cands[k]);
        g->minfo.own_candidates = own.size();
        if (!own.empty()) {
            if (ctx->d_gzip_cands.ensure((own.size() + 1) * sizeof(GzipMemberCand)) != hipSuccess || ctx->d_gzip_mspans.ensure((own.size() + 1) * sizeof(GzipSpan)) != hipSuccess) {
                return fail(ctx, RALA_HIP_ENOMEM, "device memory for the member candidates");
            }
            mspans.resize(own.size());
            HIPCHECK(hipMemcpyAsync(ctx->d_gzip_starts.p, g->starts.data(), g->n_chunks * 8, hipMemcpyHostToDevice, s));
            HIPCHECK(hipMemcpyAsync(ctx->d_gzip_cands.p, own.data(), own.size() * sizeof(GzipMemberCand), hipMemcpyHostToDevice, s));
            launch_gzip_count_members(ctx->d_bgzf_comp.p, g->end, ctx->d_gzip_starts.p, (uint32_t)g->n_chunks, (const GzipMemberCand*)ctx->d_gzip_cands.p,
                                      (uint32_t)own.size(), g->deflate_off, g->chunk, (GzipSpan*)ctx->d_gzip_mspans.p, s);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipMemcpyAsync(mspans.data(), ctx->d_gzip_mspans.p, own.size() * sizeof(GzipSpan), hipMemcpyDeviceToHost, s));
            HIPCHECK(hipStreamSynchronize(s));
        }
    }
    std::vector<uint64_t> dev(g->starts);
    if (g->c0) dev[g->c0 - 1] = kGzipNoStart;                  // (launch_gzip_count_range: the block in front of the own chunks decodes nothing)
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_starts.p, dev.data(), g->n_chunks * 8, hipMemcpyHostToDevice, s));
    launch_gzip_count_range(ctx->d_bgzf_comp.p, g->end, ctx->d_gzip_starts.p, (uint32_t)g->n_chunks, (uint32_t)g->c0, (uint32_t)g->c1,
                            (GzipSpan*)ctx->d_gzip_spans.p, s);
    HIPCHECK(hipGetLastError());
    std::vector<GzipSpan> spans(g->c1 - g->c0);
    if (!spans.empty()) HIPCHECK(hipMemcpyAsync(spans.data(), (const GzipSpan*)ctx->d_gzip_spans.p + g->c0, spans.size() * sizeof(GzipSpan), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    const uint64_t base = g->c0 ? g->c0 - 1 : 0;
    for (size_t c = 0; c < spans.size(); ++c) {
        const GzipSpan& sp = spans[c];
        spans_out[4 * c] = sp.end_bit;
        spans_out[4 * c + 1] = sp.text;
        spans_out[4 * c + 2] = (uint64_t)(uint32_t)(sp.next + base) | (uint64_t)sp.status << 32;
        spans_out[4 * c + 3] = sp.refuted;
    }
    for (size_t k = 0; k < mspans.size(); ++k) {
        const GzipSpan& sp = mspans[k];
        uint64_t* w = &spans_out[4 * (g->most + k)];
        w[0] = sp.end_bit; w[1] = sp.text; w[2] = (uint64_t)sp.next | (uint64_t)sp.status << 32; w[3] = 0;
    }
    g->tm.decode_ms = (float)(now_ms() - t0);
    ctx->d_gzip_starts.release();
    ctx->d_gzip_spans.release();
    ctx->d_gzip_cands.release();
    ctx->d_gzip_mspans.release();
    return RALA_HIP_OK;
}

// all: what the exchange of the starts gathered.  The words a part gives to the exchange of the spans: 4 per chunk of the most
// any part owns and (option gzip_members) 4 per member candidate of the most any part owns - computed by every rank from the
// list every rank found; ranks that did not find the same number of candidates (not the same file) count none: the chain
// then refuses, on every rank.
size_t rala_hip::gzip_piece_span_words(GzipPieceRun* g, const uint64_t* all, size_t stride) {
    if (g->members_mode && !g->cands_split) {
        g->cands_split = true;
        for (uint32_t p = 0; p < g->parts; ++p) g->cands_agree = g->cands_agree && all[(size_t)p * stride + 1 + g->most] == g->cands.size();
        std::vector<uint64_t> owned(g->parts, 0);
        g->cand_part.resize(g->cands.size());
        for (size_t k = 0; k < g->cands.size(); ++k) ++owned[g->cand_part[k] = part_of_bit(g, g->cands[k].deflate_bit)];
        g->most_cands = 0;
        for (uint64_t n : owned) g->most_cands = std::max(g->most_cands, n);
        if (!g->cands_agree) g->most_cands = 0;
    }
    return 4 * (size_t)(g->most + g->most_cands);
}

// c - e. all: every part's span words; the chain (the same on every rank; *valid = false: refused, nothing else was done), the
// own jobs and those the halo needs written behind a ring of identity markers, the out-window composed -> window_out: 8192 words
int rala_hip::gzip_piece_write(rala_hip_ctx* ctx, GzipPieceRun* g, const uint64_t* all, size_t stride, bool* valid, std::vector<uint64_t>& window_out) {
    hipStream_t s = ctx->stream;
    const uint64_t ring = gzip_ring_symbols();
    *valid = false;
    window_out.assign(ring / 4, 0);
    std::vector<GzipSpan> spans(g->n_chunks);
    for (uint32_t p = 0; p < g->parts; ++p) {
        const uint64_t lo = gzip_part_chunk(g->n_chunks, g->parts, p), hi = gzip_part_chunk(g->n_chunks, g->parts, p + 1);
        for (uint64_t c = lo; c < hi; ++c) {
            const uint64_t* w = all + (size_t)p * stride + 1 + 4 * (c - lo);
            spans[c] = GzipSpan{w[0], w[1], (uint32_t)w[2], (uint32_t)(w[2] >> 32), (uint32_t)w[3], 0};
        }
    }
    if (g->members_mode) {
        // every rank walks the same words: the same jobs, `first` flags, members and verdict everywhere - where a member begins
        // is the chain's to say (the trailer in front of its header), never a rank's byte range
        if (!g->cands_agree) return RALA_HIP_OK;
        std::vector<GzipSpan> mspans(g->cands.size());
        std::vector<uint64_t> seen(g->parts, 0);
        for (size_t k = 0; k < g->cands.size(); ++k) {
            const uint32_t p = g->cand_part[k];
            const uint64_t* w = all + (size_t)p * stride + 1 + 4 * (g->most + seen[p]++);
            mspans[k] = GzipSpan{w[0], w[1], (uint32_t)w[2], (uint32_t)(w[2] >> 32), 0, 0};
        }
        if (!gzip_chain_members(g->starts.data(), spans.data(), g->n_chunks, g->cands.data(), mspans.data(), g->cands.size(), g->file_n, g->crc, g->isize,
                                g->chain, g->members, &g->tm)) {
            return RALA_HIP_OK;
        }
    } else {
        if (!gzip_chain_from_spans(g->starts.data(), spans.data(), g->n_chunks, g->end, g->isize, g->chain, &g->tm)) return RALA_HIP_OK;
        g->members.assign(1, GzipMember{0, g->tm.text_bytes, g->end, g->crc, 0});
    }
    const size_t n_jobs = g->chain.size();
    std::vector<uint64_t> start_bit(n_jobs);
    std::vector<uint64_t>& first_job = g->first_job;
    first_job.assign(g->parts + 1, 0);
    for (size_t j = 0; j < n_jobs; ++j) start_bit[j] = g->chain[j].start_bit;
    if (!gzip_pieces_split(start_bit.data(), n_jobs, g->deflate_off, g->chunk, g->n_chunks, g->parts, first_job.data())) return RALA_HIP_OK;
    *valid = true;
    // where the text of every job's member begins
    g->job_floor.resize(n_jobs);
    for (size_t j = 0; j < n_jobs; ++j) g->job_floor[j] = j == 0 || g->chain[j].first ? g->chain[j].text_off : g->job_floor[j - 1];
    if (g->members_mode) ctx->gzip_members_last = g->members;
    const uint64_t text_n = g->tm.text_bytes;
    auto off_of = [&](size_t j) { return j < n_jobs ? g->chain[j].text_off : text_n; };
    g->j0 = first_job[g->part];
    g->j1 = first_job[g->part + 1];
    g->a = off_of(g->j0);
    g->b = off_of(g->j1);
    g->j2 = g->j1;
    while (g->j2 < n_jobs && off_of(g->j2) - g->b < (uint64_t)paf_halo_bytes() + 1) ++g->j2;
    g->n_w = off_of(g->j2) - g->a;
    const uint64_t own_n = g->b - g->a;
    g->info.own_jobs = g->j1 - g->j0;
    g->info.halo_jobs = g->j2 - g->j1;
    g->info.own_text_bytes = own_n;
    if (own_n >= 1ull << 38) return fail(ctx, RALA_HIP_ETOOLARGE, "a piece's text too large for one launch");
    std::vector<GzipJob> jobs(g->chain.begin() + g->j0, g->chain.begin() + g->j2);
    std::vector<uint64_t> text_off(jobs.size() + 1, ring), floors(jobs.size() + 1, 0);
    for (size_t j = 0; j < jobs.size(); ++j) {
        text_off[j] = jobs[j].text_off = ring + (jobs[j].text_off - g->a);
        // where the text of the job's member begins, in the launch's positions (one member: where the file's text does)
        const uint64_t f = g->job_floor[g->j0 + j];
        floors[j] = f + ring >= g->a ? f + ring - g->a : 0;
    }
    const uint64_t n_seg = (g->n_w + gzip_segment_bytes() - 1) / gzip_segment_bytes();
    if (n_seg >= 0xFFFFFFF0ull) return fail(ctx, RALA_HIP_ETOOLARGE, "text too large for 32-bit segment ids");
    if (ctx->d_gzip_sym.ensure(ring + g->n_w + 64) != hipSuccess || ctx->d_gzip_text.ensure(16 + g->n_w + paf_chunk_bytes() + 8192) != hipSuccess ||
        ctx->d_gzip_jobs.ensure((jobs.size() + 1) * sizeof(GzipJob)) != hipSuccess || ctx->d_gzip_off.ensure(text_off.size()) != hipSuccess ||
        ctx->d_gzip_floor.ensure(floors.size()) != hipSuccess || ctx->d_gzip_crc.ensure(n_seg + 1) != hipSuccess || ctx->d_gzip_carry.ensure(ring) != hipSuccess ||
        ctx->d_gzip_compose_stats.ensure(4) != hipSuccess) {
        return fail(ctx, RALA_HIP_ENOMEM, "device memory for a piece of the inflated text");
    }
    std::vector<uint16_t> identity(ring);
    for (uint32_t i = 0; i < ring; ++i) identity[i] = (uint16_t)(0x8000u | i);
    const double t0 = now_ms();
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_sym.p, identity.data(), ring * 2, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(ctx->d_gzip_sym.p + ring + g->n_w, 0, 128, s));
    if (!jobs.empty()) HIPCHECK(hipMemcpyAsync(ctx->d_gzip_jobs.p, jobs.data(), jobs.size() * sizeof(GzipJob), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_off.p, text_off.data(), text_off.size() * 8, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_floor.p, floors.data(), floors.size() * 8, hipMemcpyHostToDevice, s));
    launch_gzip_write(ctx->d_bgzf_comp.p, g->end, (const GzipJob*)ctx->d_gzip_jobs.p, (uint32_t)jobs.size(), ctx->d_gzip_sym.p, ctx->d_bgzf_flag.p, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    const double t1 = now_ms();
    g->tm.decode_ms += (float)(t1 - t0);
    ctx->d_bgzf_comp.release();
    // the out-window, taken at b
    uint32_t stats[4] = {0, 0, 0, 0};
    HIPCHECK(hipMemsetAsync(ctx->d_gzip_compose_stats.p, 0, 16, s));
    if (g->members_mode) {
        // (a chase ends at the floor of the member its first symbol belongs to)
        launch_gzip_window_compose_members(ctx->d_gzip_sym.p, ctx->d_gzip_off.p, ctx->d_gzip_floor.p, (uint32_t)(g->j1 - g->j0), own_n, ctx->d_gzip_carry.p,
                                           ctx->d_gzip_compose_stats.p, ctx->d_bgzf_flag.p, s);
    } else {
        launch_gzip_window_compose(ctx->d_gzip_sym.p, ctx->d_gzip_off.p, (uint32_t)(g->j1 - g->j0), own_n, ctx->d_gzip_carry.p, ctx->d_gzip_compose_stats.p,
                                   ctx->d_bgzf_flag.p, s);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(window_out.data(), ctx->d_gzip_carry.p, ring * 2, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(stats, ctx->d_gzip_compose_stats.p, 16, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    g->info.window_markers = (uint64_t)stats[0] | (uint64_t)stats[1] << 32;
    g->info.longest_chase = stats[2];
    g->info.compose_ms = (float)(now_ms() - t1);
    if (g->members_mode) {
        g->minfo.floor_stops = stats[3];
        g->minfo.compose_ms = g->info.compose_ms;
        for (const GzipMember& m : g->members) {
            const uint64_t hi = m.text_off + m.text_n;
            g->minfo.members_begun += m.text_n != 0 && m.text_off >= g->a && m.text_off < g->b;
            g->minfo.member_ends += m.text_n != 0 && hi > g->a && hi <= g->b;
        }
    }
    return RALA_HIP_OK;
}

// f - g. all: every part's out-window; the window in front of the piece composed and uploaded as the carry, windows and resolve
// as for a window of a walk: the text [a, a + n_w) to ctx->d_gzip_text + 16 with the byte in front of it ('\n' in front of the
// file's first) and newlines behind it; *flag: the inflater's.  own[0 .. 1] = CRC register and length of the own text [a, b).
// Option gzip_members: the window is masked in front of the member the piece begins in (gzip_compose_windows_masked), every
// member that lies inside the own text is proven here, and own[2 .. 6] = {head register, head length, tail register, tail
// length, the first such member that failed or ~0}: what the piece owes the members that span ranks (gzip_part_owes);
// own[0 .. 1] stay zero.
int rala_hip::gzip_piece_resolve(rala_hip_ctx* ctx, GzipPieceRun* g, const uint64_t* all, size_t stride, uint32_t* flag, uint64_t own[7]) {
    hipStream_t s = ctx->stream;
    const uint64_t ring = gzip_ring_symbols(), seg = gzip_segment_bytes();
    *flag = 0;
    for (int k = 0; k < 6; ++k) own[k] = 0;
    own[6] = ~0ull;
    std::vector<uint16_t> windows((size_t)g->parts * ring), carry(ring);
    for (uint32_t p = 0; p < g->parts; ++p) memcpy(windows.data() + (size_t)p * ring, all + (size_t)p * stride + 1, ring * 2);
    bool valid = false;
    uint8_t before = '\n';
    if (g->members_mode) {
        // every part's reach: the text between the first byte of the member its text begins in and its own first byte
        const size_t n_all = g->chain.size();
        std::vector<uint64_t> reach(g->parts, 0);
        for (uint32_t p = 0; p < g->parts; ++p) {
            const size_t j = g->first_job[p];
            if (j < n_all) reach[p] = std::min<uint64_t>(g->chain[j].text_off - g->job_floor[j], ring);
        }
        int in_front = -1;
        gzip_compose_windows_masked(windows.data(), reach.data(), g->part, carry.data(), &in_front, &valid);
        if (g->a && in_front >= 0) before = (uint8_t)in_front;
    } else {
        gzip_compose_windows(windows.data(), g->part, carry.data(), &valid);
        if (g->a && carry[ring - 1] < 0x100) before = (uint8_t)carry[ring - 1];
    }
    // (a window that is not the text's tail: refused here - and by the rank whose match it was, whose resolve meets no byte)
    if (!valid) *flag = 8;
    for (uint32_t i = 0; i < ring; ++i) if (carry[i] >= 0x100) carry[i] = 0x8000;
    const uint64_t own_n = g->b - g->a, n_w = g->n_w, n_seg = (n_w + seg - 1) / seg;
    const uint32_t n_jobs = (uint32_t)(g->j2 - g->j0);
    uint8_t* text = ctx->d_gzip_text.p + 16;
    const double t0 = now_ms();
    HIPCHECK(hipMemcpyAsync(ctx->d_gzip_sym.p, carry.data(), ring * 2, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(ctx->d_gzip_text.p, '\n', 16, s));
    HIPCHECK(hipMemcpyAsync(text - 1, &before, 1, hipMemcpyHostToDevice, s));
    launch_gzip_resolve(ctx->d_gzip_sym.p, ctx->d_gzip_off.p, ctx->d_gzip_floor.p, n_jobs, n_w, text, ctx->d_gzip_crc.p, ctx->d_bgzf_flag.p, s, ring);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemsetAsync(text + n_w, '\n', paf_chunk_bytes() + 8192 - 16, s));
    std::vector<uint32_t> seg_crc(n_seg);
    uint32_t kernel_flag = 0;
    if (n_seg) HIPCHECK(hipMemcpyAsync(seg_crc.data(), ctx->d_gzip_crc.p, n_seg * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(&kernel_flag, ctx->d_bgzf_flag.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    *flag |= kernel_flag;
    if (g->members_mode) {
        if (!*flag) { const int rc = piece_prove_members(ctx, g, text, seg_crc, own); if (rc != RALA_HIP_OK) return rc; }
        g->tm.resolve_ms = (float)(now_ms() - t0);
        ctx->d_gzip_sym.release();
        ctx->d_gzip_carry.release();
        ctx->gzip_tm = g->tm;
        ctx->gzip_pieces = g->info;
        ctx->gzip_member_pieces = g->minfo;
        if (trace_on()) {
            fprintf(stderr, "[trace] device inflate: part %u of %u of %lu gzip members (%lu header candidates found in %.2f ms, %lu counted here): chunks "
                    "[%lu, %lu) of %lu, jobs [%lu, %lu) and %lu for the halo, text [%lu, %lu) of %lu; %lu members begin and %lu end in it, %u registers "
                    "for those that span ranks; %lu own symbols through the window in front (longest chase %u hops, %u stopped at a member's floor), "
                    "compose %.2f ms; find %.2f ms, decode %.2f ms, resolve %.2f ms, the file shipped in %.1f ms\n", g->part, g->parts,
                    (unsigned long)g->members.size(), (unsigned long)g->cands.size(), g->member_find_ms, (unsigned long)g->minfo.own_candidates,
                    (unsigned long)g->c0, (unsigned long)g->c1, (unsigned long)g->n_chunks, (unsigned long)g->j0, (unsigned long)g->j1,
                    (unsigned long)(g->j2 - g->j1), (unsigned long)g->a, (unsigned long)g->b, (unsigned long)g->tm.text_bytes,
                    (unsigned long)g->minfo.members_begun, (unsigned long)g->minfo.member_ends, g->minfo.registers_sent,
                    (unsigned long)g->info.window_markers, g->info.longest_chase, g->minfo.floor_stops, g->info.compose_ms, g->tm.find_ms, g->tm.decode_ms,
                    g->tm.resolve_ms, g->ship_ms);
        }
        return RALA_HIP_OK;
    }
    // the own text's register: the whole segments' and, where b cuts one, that segment's front by gzip_piece_crc_kernel
    std::vector<uint32_t> reg;
    std::vector<uint64_t> len;
    const uint64_t whole = own_n == n_w ? n_seg : own_n / seg;
    for (uint64_t k = 0; k < whole; ++k) { reg.push_back(seg_crc[k]); len.push_back(std::min(seg, own_n - k * seg)); }
    if (!*flag && whole * seg < own_n) {
        const GzipPiece cut{whole * seg, (uint32_t)(own_n - whole * seg), 0};
        uint32_t r = 0;
        if (ctx->d_gzip_pieces.ensure(sizeof(GzipPiece)) != hipSuccess || ctx->d_gzip_piece_crc.ensure(1) != hipSuccess) {
            return fail(ctx, RALA_HIP_ENOMEM, "device memory for the piece's last segment");
        }
        HIPCHECK(hipMemcpyAsync(ctx->d_gzip_pieces.p, &cut, sizeof(cut), hipMemcpyHostToDevice, s));
        launch_gzip_piece_crc(text, (const GzipPiece*)ctx->d_gzip_pieces.p, 1, ctx->d_gzip_piece_crc.p, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(&r, ctx->d_gzip_piece_crc.p, 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        reg.push_back(r);
        len.push_back(cut.n);
    }
    own[0] = gzip_crc_register_chain(reg.data(), len.data(), reg.size());
    own[1] = own_n;
    g->tm.resolve_ms = (float)(now_ms() - t0);
    ctx->d_gzip_sym.release();
    ctx->d_gzip_carry.release();
    ctx->gzip_tm = g->tm;
    ctx->gzip_pieces = g->info;
    if (trace_on()) {
        fprintf(stderr, "[trace] device inflate: part %u of %u of one gzip member: chunks [%lu, %lu) of %lu, jobs [%lu, %lu) and %lu for the halo, text [%lu, "
                "%lu) of %lu; %lu own symbols through the window in front (longest chase %u hops), compose %.2f ms; find %.2f ms, decode %.2f ms, "
                "resolve %.2f ms, the file shipped in %.1f ms\n", g->part, g->parts, (unsigned long)g->c0, (unsigned long)g->c1, (unsigned long)g->n_chunks,
                (unsigned long)g->j0, (unsigned long)g->j1, (unsigned long)(g->j2 - g->j1), (unsigned long)g->a, (unsigned long)g->b,
                (unsigned long)g->tm.text_bytes, (unsigned long)g->info.window_markers, g->info.longest_chase, g->info.compose_ms, g->tm.find_ms,
                g->tm.decode_ms, g->tm.resolve_ms, g->ship_ms);
    }
    return RALA_HIP_OK;
}

void rala_hip::gzip_piece_text(const GzipPieceRun* g, uint64_t* own_n, uint64_t* n_w, uint64_t* file_n, float* ship_ms, uint32_t* n_readers) {
    *own_n = g->b - g->a;
    *n_w = g->n_w;
    *file_n = g->file_n;
    *ship_ms = g->ship_ms;
    *n_readers = g->n_readers;
}

// every part's {register, length} of its own text, in part order: is the text the trailer's?
bool rala_hip::gzip_piece_proven(const GzipPieceRun* g, const uint32_t* reg, const uint64_t* len, uint32_t parts) {
    uint64_t total = 0;
    for (uint32_t p = 0; p < parts; ++p) total += len[p];
    return total == g->tm.text_bytes && gzip_crc_chain(reg, len, parts) == g->crc;
}

bool rala_hip::gzip_piece_members(const GzipPieceRun* g) { return g->members_mode; }

// Option gzip_members.  all: what the last exchange gathered, part p's {head register, head length, tail register, tail length,
// locally failed member} at all[p * stride + at ..]: every member is its trailer's - those inside one rank's text by that rank's
// word, those that span ranks by the ranks' registers chained in rank order; the same verdict from the same words everywhere.
bool rala_hip::gzip_piece_members_proven(const GzipPieceRun* g, const uint64_t* all, size_t stride, size_t at) {
    const uint32_t P = g->parts;
    if (g->first_job.size() != (size_t)P + 1 || g->members.empty()) return false;
    std::vector<uint64_t> a(P), b(P), head_len(P), tail_len(P), bad_here(P);
    std::vector<uint32_t> head_reg(P), tail_reg(P);
    const size_t n_jobs = g->chain.size();
    auto off_of = [&](size_t j) { return j < n_jobs ? g->chain[j].text_off : g->tm.text_bytes; };
    for (uint32_t p = 0; p < P; ++p) {
        const uint64_t* w = all + (size_t)p * stride + at;
        a[p] = off_of(g->first_job[p]);
        b[p] = off_of(g->first_job[p + 1]);
        head_reg[p] = (uint32_t)w[0]; head_len[p] = w[1]; tail_reg[p] = (uint32_t)w[2]; tail_len[p] = w[3]; bad_here[p] = w[4];
    }
    uint64_t bad = 0;
    return gzip_members_proof(g->members.data(), g->members.size(), a.data(), b.data(), head_reg.data(), head_len.data(), tail_reg.data(), tail_len.data(),
                              bad_here.data(), P, gzip_crc_chain, &bad);
}

void rala_hip::gzip_piece_exchange_ms(rala_hip_ctx* ctx, float ms) { ctx->gzip_pieces.exchange_ms = ms; }

void rala_hip::ingest::trace_gzip(const GzipStream& g, uint64_t windows, uint64_t window) {
    const rala_hip_gzip_timings& t = g.tm;
    char in[96] = "", members[160] = "one gzip member";
    if (windows) snprintf(in, sizeof(in), " in %lu windows of at most %.3f GB of text", (unsigned long)windows, window / 1e9);
    if (g.members.size() > 1) {
        snprintf(members, sizeof(members), "%lu gzip members (%lu header candidates found in %.2f ms)", (unsigned long)g.members.size(),
                 (unsigned long)g.n_cands, g.member_find_ms);
    }
    fprintf(stderr, "[trace] device inflate: %s%s, %.3f GB compressed shipped in %.1f ms, %lu chunks (%lu with a candidate, %lu "
            "confirmed, %lu refuted), %.3f GB of text (at most %.3f GB by one wave): find %.2f ms, decode %.2f ms, resolve %.2f ms\n", members, in,
            t.compressed_bytes / 1e9, g.ship_ms, (unsigned long)t.chunks, (unsigned long)t.chunks_with_candidate, (unsigned long)t.chunks_confirmed,
            (unsigned long)t.chunks_refuted, t.text_bytes / 1e9, t.max_wave_text_bytes / 1e9, t.find_ms, t.decode_ms, t.resolve_ms);
}

extern "C" {

uint32_t rala_hip_crc32_chain(const uint32_t* reg, const uint64_t* len, uint64_t n) {
    if (n && (!reg || !len)) return 0;
    return gzip_crc_chain(reg, len, n);
}

int rala_hip_gzip_head(const uint8_t* bytes, uint64_t n, uint64_t* deflate_off, int* valid) {
    if ((!bytes && n) || !deflate_off || !valid) return RALA_HIP_EINVAL;
    *deflate_off = 0;
    *valid = gzip_head(bytes, n, deflate_off) ? 1 : 0;
    return RALA_HIP_OK;
}

int rala_hip_gzip_chain(const uint64_t* starts, const uint64_t* end_bit, const uint64_t* text, const uint32_t* next, const uint32_t* status,
                        const uint32_t* refuted, uint64_t n_chunks, uint64_t end, uint32_t isize, uint64_t cap, uint64_t* n_jobs,
                        uint64_t* start_bit, uint64_t* stop_bit, uint64_t* text_off, uint64_t* text_n, rala_hip_gzip_timings* stats, int* valid) {
    if (!n_jobs || !valid || (n_chunks && (!starts || !end_bit || !text || !next || !status || !refuted))) return RALA_HIP_EINVAL;
    std::vector<GzipSpan> spans(n_chunks);
    for (uint64_t c = 0; c < n_chunks; ++c) spans[c] = GzipSpan{end_bit[c], text[c], next[c], status[c], refuted[c], 0};
    std::vector<GzipJob> chain;
    rala_hip_gzip_timings tm = {};
    tm.chunks = n_chunks;
    *valid = gzip_chain_from_spans(starts, spans.data(), n_chunks, end, isize, chain, &tm) ? 1 : 0;
    if (stats) *stats = tm;
    *n_jobs = *valid ? chain.size() : 0;
    if (!*valid || cap < chain.size()) return RALA_HIP_OK;
    for (size_t j = 0; j < chain.size(); ++j) {
        if (start_bit) start_bit[j] = chain[j].start_bit;
        if (stop_bit) stop_bit[j] = chain[j].stop_bit;
        if (text_off) text_off[j] = chain[j].text_off;
        if (text_n) text_n[j] = chain[j].text_n;
    }
    return RALA_HIP_OK;
}

int rala_hip_gzip_chain_members(const uint64_t* starts, const uint64_t* end_bit, const uint64_t* text, const uint32_t* next, const uint32_t* status,
                                const uint32_t* refuted, uint64_t n_chunks, const uint64_t* cand_header_off, const uint64_t* cand_deflate_bit,
                                const uint32_t* cand_prev_crc, const uint32_t* cand_prev_isize, const uint64_t* cand_end_bit, const uint64_t* cand_text,
                                const uint32_t* cand_next, const uint32_t* cand_status, uint64_t n_cands, uint64_t file_n, uint32_t last_crc,
                                uint32_t last_isize, uint64_t cap, uint64_t* n_jobs, uint64_t* start_bit, uint64_t* stop_bit, uint64_t* text_off,
                                uint64_t* text_n, uint32_t* first, uint64_t member_cap, uint64_t* n_members, uint64_t* member_text_off,
                                uint64_t* member_text_n, uint32_t* member_crc32, rala_hip_gzip_timings* stats, int* valid) {
    if (!n_jobs || !n_members || !valid || (n_chunks && (!starts || !end_bit || !text || !next || !status || !refuted)) ||
        (n_cands && (!cand_header_off || !cand_deflate_bit || !cand_prev_crc || !cand_prev_isize || !cand_end_bit || !cand_text || !cand_next || !cand_status))) {
        return RALA_HIP_EINVAL;
    }
    std::vector<GzipSpan> spans(n_chunks), mspans(n_cands);
    std::vector<GzipMemberCand> cands(n_cands);
    for (uint64_t c = 0; c < n_chunks; ++c) spans[c] = GzipSpan{end_bit[c], text[c], next[c], status[c], refuted[c], 0};
    for (uint64_t k = 0; k < n_cands; ++k) {
        cands[k] = GzipMemberCand{cand_header_off[k], cand_deflate_bit[k], cand_prev_crc[k], cand_prev_isize[k]};
        mspans[k] = GzipSpan{cand_end_bit[k], cand_text[k], cand_next[k], cand_status[k], 0, 0};
    }
    std::vector<GzipJob> chain;
    std::vector<GzipMember> members;
    rala_hip_gzip_timings tm = {};
    tm.chunks = n_chunks;
    *valid = gzip_chain_members(starts, spans.data(), n_chunks, cands.data(), mspans.data(), n_cands, file_n, last_crc, last_isize, chain, members, &tm) ? 1 : 0;
    if (stats) *stats = tm;
    *n_jobs = *valid ? chain.size() : 0;
    *n_members = *valid ? members.size() : 0;
    if (!*valid) return RALA_HIP_OK;
    for (size_t j = 0; j < chain.size() && cap >= chain.size(); ++j) {
        if (start_bit) start_bit[j] = chain[j].start_bit;
        if (stop_bit) stop_bit[j] = chain[j].stop_bit;
        if (text_off) text_off[j] = chain[j].text_off;
        if (text_n) text_n[j] = chain[j].text_n;
        if (first) first[j] = chain[j].first;
    }
    for (size_t m = 0; m < members.size() && member_cap >= members.size(); ++m) {
        if (member_text_off) member_text_off[m] = members[m].text_off;
        if (member_text_n) member_text_n[m] = members[m].text_n;
        if (member_crc32) member_crc32[m] = members[m].crc;
    }
    return RALA_HIP_OK;
}

int rala_hip_gzip_find_members(rala_hip_ctx* ctx, const uint8_t* bytes, uint64_t n, uint64_t cap, uint64_t* n_found, uint64_t* header_off,
                               uint64_t* deflate_off) {
    if (!ctx || !n_found || (!bytes && n)) return RALA_HIP_EINVAL;
    *n_found = 0;
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (ctx->d_bgzf_comp.ensure(n + 64) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the bytes");
    struct Release {
        rala_hip_ctx* ctx;
        ~Release() { ctx->d_bgzf_comp.release(); ctx->d_gzip_cands.release(); ctx->d_gzip_tile.release(); }
    } release{ctx};
    if (n) HIPCHECK(hipMemcpyAsync(ctx->d_bgzf_comp.p, bytes, n, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(ctx->d_bgzf_comp.p + n, 0, 64, s));
    uint64_t found = 0;
    const int rc = gzip_member_find(ctx, ctx->d_bgzf_comp.p, n, &found);
    if (rc != RALA_HIP_OK) return rc;
    *n_found = found;
    if (!found || cap < found) return RALA_HIP_OK;
    std::vector<GzipMemberCand> cands(found);
    HIPCHECK(hipMemcpy(cands.data(), ctx->d_gzip_cands.p, found * sizeof(GzipMemberCand), hipMemcpyDeviceToHost));
    for (uint64_t k = 0; k < found; ++k) {
        if (header_off) header_off[k] = cands[k].header_off;
        if (deflate_off) deflate_off[k] = cands[k].deflate_bit / 8;
    }
    return RALA_HIP_OK;
}

int rala_hip_gzip_pieces(const uint64_t* job_start_bit, uint64_t n_jobs, uint64_t deflate_off, uint64_t chunk_bytes, uint64_t n_chunks,
                         uint32_t parts, uint64_t* first_job) {
    if (!first_job || (!job_start_bit && n_jobs)) return RALA_HIP_EINVAL;
    return gzip_pieces_split(job_start_bit, n_jobs, deflate_off, chunk_bytes, n_chunks, parts, first_job) ? RALA_HIP_OK : RALA_HIP_EINVAL;
}

int rala_hip_gzip_compose_windows(const uint16_t* out_windows, uint32_t parts, uint32_t part, uint16_t* in_window, int* valid) {
    static_assert(kGzipNothing == RALA_HIP_GZIP_NOTHING, "the header names the code");
    if (!out_windows || !in_window || !valid || part >= parts) return RALA_HIP_EINVAL;
    bool ok = false;
    gzip_compose_windows(out_windows, part, in_window, &ok);
    *valid = ok ? 1 : 0;
    return RALA_HIP_OK;
}

int rala_hip_gzip_compose_windows_masked(const uint16_t* out_windows, uint32_t parts, const uint64_t* reach, uint32_t part, uint16_t* in_window,
                                         int* before, int* valid) {
    if (!out_windows || !reach || !in_window || !before || !valid || part >= parts) return RALA_HIP_EINVAL;
    bool ok = false;
    gzip_compose_windows_masked(out_windows, reach, part, in_window, before, &ok);
    *valid = ok ? 1 : 0;
    return RALA_HIP_OK;
}

int rala_hip_gzip_members_proof(const uint64_t* member_text_off, const uint64_t* member_text_n, const uint32_t* member_crc32, uint64_t n_members,
                                const uint64_t* part_begin, const uint64_t* part_end, const uint32_t* head_reg, const uint64_t* head_len,
                                const uint32_t* tail_reg, const uint64_t* tail_len, const uint64_t* local_bad, uint32_t parts, uint64_t* bad_member,
                                int* valid) {
    if (!member_text_off || !member_text_n || !member_crc32 || !n_members || !part_begin || !part_end || !head_reg || !head_len || !tail_reg || !tail_len ||
        !local_bad || !parts || !bad_member || !valid) {
        return RALA_HIP_EINVAL;
    }
    std::vector<GzipMember> members(n_members);
    for (uint64_t m = 0; m < n_members; ++m) members[m] = GzipMember{member_text_off[m], member_text_n[m], 0, member_crc32[m], 0};
    *valid = gzip_members_proof(members.data(), n_members, part_begin, part_end, head_reg, head_len, tail_reg, tail_len, local_bad, parts, gzip_crc_chain,
                                bad_member) ? 1 : 0;
    return RALA_HIP_OK;
}

int rala_hip_get_gzip_member_pieces_info(rala_hip_ctx* ctx, rala_hip_gzip_member_pieces_info* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->gzip_member_pieces;
    return RALA_HIP_OK;
}

int rala_hip_get_gzip_pieces_info(rala_hip_ctx* ctx, rala_hip_gzip_pieces_info* out) {
    if (!ctx || !out) return RALA_HIP_EINVAL;
    *out = ctx->gzip_pieces;
    return RALA_HIP_OK;
}

int rala_hip_get_gzip_members(rala_hip_ctx* ctx, uint64_t* n, uint64_t cap, uint64_t* text_off, uint64_t* text_n, uint32_t* crc32) {
    if (!ctx || !n) return RALA_HIP_EINVAL;
    const std::vector<GzipMember>& m = ctx->gzip_members_last;
    *n = m.size();
    for (size_t k = 0; k < m.size() && cap >= m.size(); ++k) {
        if (text_off) text_off[k] = m[k].text_off;
        if (text_n) text_n[k] = m[k].text_n;
        if (crc32) crc32[k] = m[k].crc;
    }
    return RALA_HIP_OK;
}

}  // extern "C"
