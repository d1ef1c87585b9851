// BGZF files on the device: the member index made while the file is read, the members that cover a range of the text
// shipped and inflated (inflate_kernels.hip: launch_bgzf_inflate).
#include <atomic>

#include "ingest_common.h"

using namespace rala_hip;
using namespace rala_hip::ingest;

int rala_hip::ingest::bgzf_open(rala_hip_ctx* ctx, int fd, uint64_t file_n, const char* path, uint32_t threads, uint64_t window, BgzfFile& f,
                                bool* valid) {
    *valid = false;
    f.fd = fd;
    f.file_n = file_n;
    if (file_n < 18) return RALA_HIP_OK;
    const double t0 = now_ms();
    f.resident = file_n <= window;
    if (f.resident && ctx->d_bgzf_comp.ensure(file_n + 64) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
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
    if (shipped || edge_failed) return fail(ctx, RALA_HIP_EDEVICE, std::string("reading / copying ") + path + " failed");
    uint8_t tail[4];
    if (pread(fd, tail, 4, (off_t)(file_n - 4)) != 4) return fail(ctx, RALA_HIP_EDEVICE, std::string("reading ") + path + " failed");
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

int rala_hip::ingest::bgzf_open_piece(rala_hip_ctx* ctx, int fd, uint64_t file_n, const char* path, uint32_t threads, uint64_t lo, uint64_t hi,
                                      uint64_t follow_text, BgzfFile& f, BgzfPiece* piece, uint64_t* own_text, bool* valid) {
    *valid = false;
    *own_text = 0;
    f.fd = fd;
    f.file_n = file_n;
    f.resident = true;
    f.comp_origin = lo;
    hi = std::min(hi, file_n);
    lo = std::min(lo, hi);
    piece->begin = piece->end = lo;
    piece->empty = 1;
    if (hi == lo) { *valid = true; return RALA_HIP_OK; }
    const double t0 = now_ms();
    const uint64_t len = hi - lo;
    // (room for the member across hi and a usual halo's members at once; more is made below where they need more)
    if (ctx->d_bgzf_comp.ensure(len + 4 * 65536 + 64) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
    const std::string read_failed = std::string("reading / copying ") + path + " failed";
    const uint64_t n_blocks = (len + kBlockBytes - 1) / kBlockBytes;
    std::vector<std::vector<BgzfCand>> cand(n_blocks);
    std::atomic<int> edge_failed(0);
    const BlockScan scan = [&](uint64_t b, const uint8_t* bytes, size_t n) {
        const uint64_t off = lo + b * kBlockBytes;
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
    const int shipped = ship_file(fd, lo, len, ctx->d_bgzf_comp.p, ctx->device, threads, &scan, []() { return true; }, &f.n_readers);
    if (shipped || edge_failed) return fail(ctx, RALA_HIP_EDEVICE, read_failed);
    uint8_t tail[4] = {0, 0, 0, 0};
    if (file_n >= 4 && pread(fd, tail, 4, (off_t)(file_n - 4)) != 4) return fail(ctx, RALA_HIP_EDEVICE, read_failed);
    // the candidate at an offset behind the range: the 4 bytes in front of it, its fixed part, then its extra field
    bool io_failed = false;
    auto next = [&](uint64_t o, BgzfCand* c) {
        if (o < 4 || o + 12 > file_n) return false;
        std::vector<uint8_t> h(16);
        if (pread(fd, h.data(), 16, (off_t)(o - 4)) != 16) { io_failed = true; return false; }
        const uint64_t reach = std::min<uint64_t>(12 + (h[14] | (uint64_t)h[15] << 8), file_n - o);
        h.resize(4 + reach);
        if (reach > 12 && pread(fd, h.data() + 16, reach - 12, (off_t)(o + 12)) != (ssize_t)(reach - 12)) { io_failed = true; return false; }
        std::vector<BgzfCand> v;
        bgzf_scan(h.data() + 4, 1, o, file_n, [&](uint64_t q) { return h[q + 4 - o]; }, v);
        if (v.empty()) return false;
        *c = v[0];
        return true;
    };
    std::vector<BgzfMember> members;
    const bool chained = bgzf_walk_range(cand, lo, hi, file_n, le32(tail), next, members, piece);
    if (io_failed) return fail(ctx, RALA_HIP_EDEVICE, read_failed);
    if (!chained) return RALA_HIP_OK;
    f.n_members = members.size();
    if (piece->empty) { *valid = true; return RALA_HIP_OK; }
    uint64_t text = 0;
    for (const BgzfMember& m : members) text += m.isize;
    *own_text = text;
    // the members behind the piece, as far as the text wanted of them reaches (checked like the piece's own: the piece that
    // owns them will refuse what is refused here)
    uint64_t o = piece->end;
    for (uint64_t got = 0; o < file_n && got < follow_text;) {
        BgzfCand c;
        uint8_t isize[4];
        if (!next(o, &c) || c.bsize == 0 || o + c.bsize > file_n) {
            if (io_failed) return fail(ctx, RALA_HIP_EDEVICE, read_failed);
            return RALA_HIP_OK;
        }
        if (pread(fd, isize, 4, (off_t)(o + c.bsize - 4)) != 4) return fail(ctx, RALA_HIP_EDEVICE, read_failed);
        BgzfMember m;
        m.off = o; m.bsize = c.bsize; m.hdr = c.hdr; m.isize = le32(isize); m.text_off = text;
        if (m.isize > 65536) return RALA_HIP_OK;
        members.push_back(m);
        text += m.isize;
        got += m.isize;
        o += c.bsize;
    }
    // bytes [hi, o): the rest of the member across hi and the members that follow
    if (o > hi) {
        std::vector<uint8_t> rest(o - hi);
        for (uint64_t got = 0; got < rest.size();) {
            const ssize_t r = pread(fd, rest.data() + got, rest.size() - got, (off_t)(hi + got));
            if (r <= 0) return fail(ctx, RALA_HIP_EDEVICE, read_failed);
            got += (uint64_t)r;
        }
        if (ctx->d_bgzf_comp.grow(len, o - lo + 64) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
        HIPCHECK(hipMemcpy(ctx->d_bgzf_comp.p + len, rest.data(), rest.size(), hipMemcpyHostToDevice));
    }
    for (const BgzfMember& m : members) if (m.isize) f.jobs.push_back(m);
    f.text_n = text;
    f.shipped = o - lo;
    f.ship_ms = (float)(now_ms() - t0);
    *valid = true;
    return RALA_HIP_OK;
}

int rala_hip::ingest::bgzf_text_range(rala_hip_ctx* ctx, BgzfFile& f, uint64_t lo, uint64_t n_avail, uint64_t cap, int pad, uint32_t threads,
                                      const std::function<bool()>& meanwhile, const char* room, TextArrival* out) {
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
    if (ctx->d_paf_text.ensure(size) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the file's text");
    uint64_t comp_base = 0;
    if (!f.resident && j1 > j0) {
        comp_base = f.jobs[j0].off;
        const uint64_t c_len = f.jobs[j1 - 1].off + f.jobs[j1 - 1].bsize - comp_base;
        if (ctx->d_bgzf_comp.ensure(c_len + 64) != hipSuccess) return fail(ctx, RALA_HIP_ENOMEM, "device memory for the compressed file");
        const int shipped = ship_file(f.fd, comp_base, c_len, ctx->d_bgzf_comp.p, ctx->device, threads, nullptr, meanwhile, &f.n_readers);
        if (shipped == 2) return fail(ctx, RALA_HIP_ENOMEM, room);
        if (shipped) return fail(ctx, RALA_HIP_EDEVICE, "reading / copying the compressed file failed");
        f.shipped += c_len;
    } else if (!meanwhile()) {
        return fail(ctx, RALA_HIP_ENOMEM, room);
    }
    out->t_ship = now_ms();
    std::vector<BgzfJob> jobs(j1 - j0);
    for (size_t j = j0; j < j1; ++j) {
        const BgzfMember& m = f.jobs[j];
        BgzfJob& J = jobs[j - j0];
        J.comp_off = m.off + m.hdr - (f.resident ? f.comp_origin : comp_base);
        J.text_off = m.text_off - base;
        J.deflate_len = m.bsize - m.hdr - 8;
        J.isize = m.isize;
    }
    uint32_t flag = 0;
    if (!jobs.empty()) {
        HIPCHECK(ctx->d_bgzf_jobs.ensure(jobs.size() * sizeof(BgzfJob)));
        HIPCHECK(ctx->d_bgzf_flag.ensure(1));
        HIPCHECK(hipMemcpyAsync(ctx->d_bgzf_jobs.p, jobs.data(), jobs.size() * sizeof(BgzfJob), hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemsetAsync(ctx->d_bgzf_flag.p, 0, 4, s));
        launch_bgzf_inflate(ctx->d_bgzf_comp.p, (const BgzfJob*)ctx->d_bgzf_jobs.p, (uint32_t)jobs.size(), ctx->d_paf_text.p, size, ctx->d_bgzf_flag.p, s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(&flag, ctx->d_bgzf_flag.p, 4, hipMemcpyDeviceToHost, s));
    }
    uint8_t* const text = ctx->d_paf_text.p + shift;
    HIPCHECK(hipMemsetAsync(text + n_avail, pad, cap - n_avail, s));
    HIPCHECK(hipStreamSynchronize(s));
    out->t1 = now_ms();
    f.inflate_ms += (float)(out->t1 - out->t_ship);
    if (flag) ctx->d_paf_text.release();
    out->text = text;
    out->flag = flag;
    return RALA_HIP_OK;
}

extern "C" int rala_hip_bgzf_index(const uint8_t* bytes, uint64_t n, uint64_t block_bytes, uint64_t cap, uint64_t* n_members, uint64_t* file_off,
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

extern "C" int rala_hip_bgzf_index_range(const uint8_t* bytes, uint64_t n, uint64_t lo, uint64_t hi, uint64_t block_bytes, uint64_t cap,
                                         uint64_t* n_members, uint64_t* file_off, uint32_t* comp_bytes, uint32_t* text_bytes, uint64_t* begin,
                                         uint64_t* end, int* empty, int* valid) {
    if ((!bytes && n) || !n_members || !begin || !end || !empty || !valid) return RALA_HIP_EINVAL;
    std::vector<BgzfMember> m;
    BgzfPiece piece;
    *valid = bgzf_index_range_bytes(bytes, n, lo, hi, block_bytes ? block_bytes : kBlockBytes, m, &piece) ? 1 : 0;
    *begin = piece.begin;
    *end = piece.end;
    *empty = (int)piece.empty;
    *n_members = *valid ? m.size() : 0;
    if (!*valid || cap < m.size()) return RALA_HIP_OK;
    for (size_t i = 0; i < m.size(); ++i) {
        if (file_off) file_off[i] = m[i].off;
        if (comp_bytes) comp_bytes[i] = m[i].bsize;
        if (text_bytes) text_bytes[i] = m[i].isize;
    }
    return RALA_HIP_OK;
}

extern "C" int rala_hip_bgzf_pieces_chain(const uint64_t* begin, const uint64_t* end, const int* empty, uint32_t n_pieces, uint64_t file_bytes) {
    if (!begin || !end || !empty) return 0;
    std::vector<BgzfPiece> p(n_pieces);
    for (uint32_t k = 0; k < n_pieces; ++k) { p[k].begin = begin[k]; p[k].end = end[k]; p[k].empty = empty[k] ? 1u : 0u; }
    return bgzf_pieces_chain(p.data(), p.size(), file_bytes) ? 1 : 0;
}
