// What the device ingest decides on the host from bytes it does not trust - a file's first bytes, the member headers of a
// BGZF file, the header of a gzip member, the chain through the chunks the device counted: pure functions, no device header.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gzip_types.h"
#include "rala_hip.h"

namespace rala_hip {
namespace ingest {

inline uint32_t le32(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// ---- BGZF: the member index -------------------------------------------------------------------
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
inline bool bgzf_head(const uint8_t* h, uint64_t n) {
    return n >= 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) != 0 && h[10] == 6 && h[11] == 0 && h[12] == 'B' &&
           h[13] == 'C' && h[14] == 2 && h[15] == 0;
}

// What a file is by its first 18 bytes (n: those of them it has): BGZF, any other gzip file (the magic alone), or text.
enum TextKind { kTextPlain = 0, kTextBgzf = 1, kTextGzip = 2 };
inline TextKind sniff(const uint8_t* h, uint64_t n) {
    if (n < 2 || h[0] != 0x1f || h[1] != 0x8b) return kTextPlain;
    return bgzf_head(h, n) ? kTextBgzf : kTextGzip;
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
inline bool bgzf_walk(const std::vector<std::vector<BgzfCand>>& blocks, uint64_t file_n, uint32_t tail, std::vector<BgzfMember>& members) {
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

// the index of a file in memory, scanned in blocks of block_bytes (what the readers do with their staging blocks)
inline bool bgzf_index_bytes(const uint8_t* bytes, uint64_t n, uint64_t block_bytes, std::vector<BgzfMember>& members) {
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

// ---- BGZF: a file in pieces by compressed byte range (a rank's share of a sharded run, a context's share of the -s file) ----
// Piece [lo, hi) of the file holds the members whose header BEGINS in it.  begin: its first member's offset; end: where its
// chain arrived (>= hi); empty: no header begins in the range.
struct BgzfPiece {
    uint64_t begin = 0, end = 0;
    uint32_t empty = 1;
};

// The chain of a piece's members through the candidates that begin in [lo, hi) (in file order; candidates behind hi are not
// looked at): from the FIRST candidate of the range until the chain reaches an offset >= hi, where there must be a candidate
// - next(o, &c): the candidate at offset o < file_n, false: none - or the file's end (tail: the file's last 4 bytes).  The
// members' text offsets count from the piece's first member.  false: what bgzf_walk refuses - and a piece never tries to be
// cleverer than that: a false candidate that starts the chain (a header-shaped string inside the member in front) is not
// stepped over, the pieces then do not join (bgzf_pieces_chain) and the host reader decides.
template <class Next>
bool bgzf_walk_range(const std::vector<std::vector<BgzfCand>>& blocks, uint64_t lo, uint64_t hi, uint64_t file_n, uint32_t tail,
                     const Next& next, std::vector<BgzfMember>& members, BgzfPiece* piece) {
    members.clear();
    piece->begin = piece->end = lo;
    piece->empty = 1;
    size_t b = 0, i = 0;
    auto seek = [&](uint64_t o) {
        while (b < blocks.size() && (i >= blocks[b].size() || blocks[b][i].pos < o)) {
            if (i >= blocks[b].size()) { ++b; i = 0; } else { ++i; }
        }
        return b < blocks.size();
    };
    if (!seek(lo) || blocks[b][i].pos >= hi) return true;
    uint64_t o = blocks[b][i].pos;
    piece->begin = piece->end = o;
    piece->empty = 0;
    while (o < hi) {
        piece->end = o;
        if (!seek(o)) return false;
        const BgzfCand& c = blocks[b][i];
        if (c.pos != o || c.bsize == 0 || o + c.bsize > file_n) return false;
        if (!members.empty()) members.back().isize = c.prev_isize;
        BgzfMember m;
        m.off = o; m.bsize = c.bsize; m.hdr = c.hdr; m.isize = 0; m.text_off = 0;
        members.push_back(m);
        o += c.bsize;
    }
    piece->end = o;
    if (o == file_n) {
        members.back().isize = tail;
    } else {
        BgzfCand c;
        if (!next(o, &c)) return false;
        members.back().isize = c.prev_isize;
    }
    uint64_t t = 0;
    for (BgzfMember& m : members) {
        if (m.isize > 65536) return false;
        m.text_off = t;
        t += m.isize;
    }
    return true;
}

// Do the pieces of a file of file_n bytes, in order, form one chain from offset 0 to its end?  Piece 0 begins at 0, every
// non-empty piece begins where the non-empty one in front of it ended, the last one ends at the file's end.
inline bool bgzf_pieces_chain(const BgzfPiece* pieces, size_t n, uint64_t file_n) {
    if (!n || pieces[0].empty || pieces[0].begin != 0) return false;
    uint64_t at = 0;
    for (size_t k = 0; k < n; ++k) {
        if (pieces[k].empty) continue;
        if (pieces[k].begin != at || pieces[k].end <= at) return false;
        at = pieces[k].end;
    }
    return at == file_n;
}

// the candidate at offset o of a file in memory, if there is one
inline bool bgzf_cand_at(const uint8_t* bytes, uint64_t n, uint64_t o, BgzfCand* c) {
    if (o >= n) return false;
    std::vector<BgzfCand> v;
    bgzf_scan(bytes + o, 1, o, n, [&](uint64_t q) { return bytes[q]; }, v);
    if (v.empty()) return false;
    *c = v[0];
    return true;
}

// piece [lo, hi) of a file in memory, scanned in blocks of block_bytes from lo (the piece at offset 0 wants the first header
// to be what the host reader's is_bgzf recognises, as bgzf_index_bytes does)
inline bool bgzf_index_range_bytes(const uint8_t* bytes, uint64_t n, uint64_t lo, uint64_t hi, uint64_t block_bytes,
                                   std::vector<BgzfMember>& members, BgzfPiece* piece) {
    hi = std::min(hi, n);
    lo = std::min(lo, hi);
    members.clear();
    piece->begin = piece->end = lo;
    piece->empty = 1;
    if (lo == 0 && hi > 0 && !bgzf_head(bytes, n)) return false;
    const uint64_t n_blocks = (hi - lo + block_bytes - 1) / block_bytes;
    std::vector<std::vector<BgzfCand>> cand(n_blocks);
    auto at = [&](uint64_t q) { return bytes[q]; };
    for (uint64_t b = 0; b < n_blocks; ++b) {
        const uint64_t off = lo + b * block_bytes;
        bgzf_scan(bytes + off, std::min(block_bytes, hi - off), off, n, at, cand[b]);
    }
    return bgzf_walk_range(cand, lo, hi, n, n >= 4 ? le32(bytes + n - 4) : 0,
                           [&](uint64_t o, BgzfCand* c) { return bgzf_cand_at(bytes, n, o, c); }, members, piece);
}

// ---- a single-member gzip file (gzip, pigz, Python's gzip) ---------------------------------------------------------
// The header of a gzip member (RFC 1952 2.3) in the first n bytes of a file: where its deflate bytes begin.  false: not a
// header inflate would take (magic, CM != 8, reserved flag bits) or one that does not end within the n bytes.
inline bool gzip_head(const uint8_t* h, uint64_t n, uint64_t* deflate_off) {
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

// The chain of true chunks from chunk 0 through what the device found and counted (starts[c], spans[c], c < n_chunks:
// launch_gzip_find / launch_gzip_count), their text offsets from the text's start, and the counters of `tm` that speak of
// the chain.  The host's only defence against what the device made of an untrusted file - false, the stream cannot be
// proven: a chunk on the chain that is invalid or has no start, a `next` that does not lead forward to a chunk there is,
// a final block that does not end in the byte in front of the trailer (`end`), a text whose size is not ISIZE modulo 2^32.
inline bool gzip_chain_from_spans(const uint64_t* starts, const GzipSpan* spans, uint64_t n_chunks, uint64_t end, uint32_t isize,
                                  std::vector<GzipJob>& chain, rala_hip_gzip_timings* tm) {
    chain.clear();
    if (!n_chunks) return false;
    for (uint64_t c = 1; c < n_chunks; ++c) tm->chunks_with_candidate += starts[c] != kGzipNoStart;
    uint64_t text_n = 0, end_bit = 0;
    for (uint64_t c = 0;;) {
        const GzipSpan& sp = spans[c];
        if (sp.status > 1 || (sp.status == 0 && (sp.next <= c || sp.next >= n_chunks))) return false;
        GzipJob j;
        j.start_bit = starts[c];
        j.stop_bit = sp.status == 0 ? starts[sp.next] : kGzipNoStart;
        j.text_off = text_n;
        j.text_n = sp.text;
        j.first = chain.empty() ? 1u : 0u;
        j.pad = 0;
        chain.push_back(j);
        text_n += sp.text;
        tm->chunks_refuted += sp.refuted;
        tm->max_wave_text_bytes = std::max<uint64_t>(tm->max_wave_text_bytes, sp.text);
        if (sp.status == 1) { end_bit = sp.end_bit; break; }
        c = sp.next;
    }
    tm->chunks_confirmed = chain.size() - 1;
    tm->text_bytes = text_n;
    return end_bit / 8 + (end_bit % 8 != 0) == end && (uint32_t)text_n == isize;
}

// ---- a single-member gzip stream over the ranks of a sharded run (option gzip_in_pieces) ------------------------------------
// Part k of `parts` owns the chunks [gzip_part_chunk(k), gzip_part_chunk(k + 1)): n_chunks k / parts, except that chunk 0 -
// whose start is the stream's, not one to be found - is always part 0's.
inline uint64_t gzip_part_chunk(uint64_t n_chunks, uint32_t parts, uint32_t k) {
    if (k == 0) return 0;
    if (k >= parts) return n_chunks;
    return std::min(n_chunks, std::max<uint64_t>(1, (uint64_t)((unsigned __int128)n_chunks * k / parts)));
}

// A job of the chain belongs to the part whose chunk range holds the chunk its first bit lies in; the chain ascends, so part
// k's jobs are one run [first_job[k], first_job[k + 1]) - an empty one where no block start was found in its chunks (a stream of
// fixed or stored blocks: all of it part 0's).  false: no parts, no chunks, a first bit in front of the deflate bytes, starts
// that do not ascend.
inline bool gzip_pieces_split(const uint64_t* job_start_bit, uint64_t n_jobs, uint64_t deflate_off, uint64_t chunk_bytes, uint64_t n_chunks,
                              uint32_t parts, uint64_t* first_job) {
    if (!parts || !chunk_bytes || (n_jobs && !n_chunks)) return false;
    uint32_t k = 0;
    first_job[0] = 0;
    for (uint64_t j = 0; j < n_jobs; ++j) {
        const uint64_t byte = job_start_bit[j] / 8;
        if (byte < deflate_off || (j && job_start_bit[j] <= job_start_bit[j - 1])) return false;
        const uint64_t c = std::min((byte - deflate_off) / chunk_bytes, n_chunks - 1);
        while (k + 1 < parts && c >= gzip_part_chunk(n_chunks, parts, k + 1)) first_job[++k] = j;
    }
    while (k < parts) first_job[++k] = n_jobs;
    return true;
}

// The window in front of a part - the 32 768 bytes of text that precede its first own byte - from the parts' OUT-windows:
// out_windows[r * 32768 + i] is the symbol 32 768 - i in front of the end of part r's own text, a byte or 0x8000 | k = "entry k
// of the window in front of part r" (what gzip_window_compose_kernel writes).  W_0 is nothing at all; W_{r+1}[i] = out_r[i] where
// that is a byte, else W_r[out_r[i] & 0x7FFF].  in_window = W_part: bytes, and kGzipNothing where the file's text has not begun.
// 0x8000 | 0 is a marker like any other, so "nothing" has a code that is neither a byte nor a marker.  *valid = false: an entry
// that is neither, or nothing BEHIND a byte - a window is the text's tail, nothing can only stand in front of all its bytes;
// behind one it is what a match copied from in front of the text's first byte, which zlib refuses.
constexpr uint32_t kGzipWindow = 32768;
constexpr uint16_t kGzipNothing = 0x4000;
inline void gzip_compose_windows(const uint16_t* out_windows, uint32_t part, uint16_t* in_window, bool* valid) {
    std::vector<uint16_t> w(kGzipWindow, kGzipNothing), next(kGzipWindow);
    bool ok = true;
    for (uint32_t r = 0; r < part; ++r) {
        const uint16_t* o = out_windows + (size_t)r * kGzipWindow;
        for (uint32_t i = 0; i < kGzipWindow; ++i) {
            const uint16_t s = o[i];
            if (s < 0x100) next[i] = s;
            else if (s & 0x8000) next[i] = w[s & 0x7FFF];
            else { next[i] = kGzipNothing; ok = false; }
        }
        w.swap(next);
    }
    bool byte_seen = false;
    for (uint32_t i = 0; i < kGzipWindow; ++i) {
        if (w[i] != kGzipNothing) byte_seen = true;
        else if (byte_seen) ok = false;
        in_window[i] = w[i];
    }
    *valid = ok;
}

// ---- a gzip file of several members (cat a.gz b.gz, pigz -i, appended files) ------------------------------------------------
// The same walk through a file whose members follow each other as gzread walks them (reference src/graph.cpp:190-224): besides
// the chunks, the member headers the device found (cands[k], ascending header_off: launch_gzip_member_find) and what it counted
// from each one's first block (mspans[k], decoded as a stream's first chunk).  Where a final block ends, at bit e, the member's
// trailer lies at t = ceil(e / 8): the member's text size must be the ISIZE at t + 4 modulo 2^32; with t + 8 the file's end
// (last_crc, last_isize: the file's last 8 bytes) the walk is done, otherwise a candidate with header_off == t + 8 must exist -
// the 8 bytes in front of it are that trailer - and the walk goes on at its span.  A member is entered in no other way, so a
// candidate that is no header (a magic inside deflate bytes) is never looked at.  false: what gzip_chain_from_spans refuses,
// bytes behind a trailer that are no header, a cut member, an end_bit or a candidate that does not lead forward.
// chain: first = 1 on every member's first job; members: text range, trailer and CRC32 of each, empty ones included.
inline bool gzip_chain_members(const uint64_t* starts, const GzipSpan* spans, uint64_t n_chunks, const GzipMemberCand* cands,
                               const GzipSpan* mspans, uint64_t n_cands, uint64_t file_n, uint32_t last_crc, uint32_t last_isize,
                               std::vector<GzipJob>& chain, std::vector<GzipMember>& members, rala_hip_gzip_timings* tm) {
    chain.clear();
    members.clear();
    if (!n_chunks || file_n < 8) return false;
    for (uint64_t c = 1; c < n_chunks; ++c) tm->chunks_with_candidate += starts[c] != kGzipNoStart;
    uint64_t text_n = 0, member_off = 0, c = 0, start_bit = starts[0];
    const GzipSpan* sp = &spans[0];
    bool on_chunk = true, first = true;
    for (;;) {
        if (sp->status > 1) return false;
        GzipJob j;
        j.start_bit = start_bit;
        j.stop_bit = kGzipNoStart;
        j.text_off = text_n;
        j.text_n = sp->text;
        j.first = first ? 1u : 0u;
        j.pad = 0;
        text_n += sp->text;
        tm->chunks_refuted += sp->refuted;
        tm->max_wave_text_bytes = std::max<uint64_t>(tm->max_wave_text_bytes, sp->text);
        if (sp->status == 0) {
            const uint64_t nx = sp->next;
            if (nx >= n_chunks || (on_chunk && nx <= c) || starts[nx] == kGzipNoStart || starts[nx] <= start_bit) return false;
            j.stop_bit = starts[nx];
            chain.push_back(j);
            c = nx;
            sp = &spans[nx];
            start_bit = starts[nx];
            on_chunk = true;
            first = false;
            continue;
        }
        chain.push_back(j);
        const uint64_t e = sp->end_bit;
        if (e <= start_bit) return false;
        const uint64_t t = e / 8 + (e % 8 != 0);
        if (t > file_n || file_n - t < 8) return false;                     // (a member that is cut)
        GzipMember m;
        m.text_off = member_off;
        m.text_n = text_n - member_off;
        m.trailer_off = t;
        m.pad = 0;
        if (t + 8 == file_n) {
            if ((uint32_t)m.text_n != last_isize) return false;
            m.crc = last_crc;
            members.push_back(m);
            break;
        }
        const GzipMemberCand* const k = std::lower_bound(cands, cands + n_cands, t + 8, [](const GzipMemberCand& a, uint64_t off) { return a.header_off < off; });
        if (k == cands + n_cands || k->header_off != t + 8 || k->deflate_bit < 8 * (t + 8 + 10)) return false;
        if ((uint32_t)m.text_n != k->prev_isize) return false;
        m.crc = k->prev_crc;
        members.push_back(m);
        member_off = text_n;
        sp = &mspans[k - cands];
        start_bit = k->deflate_bit;
        on_chunk = false;
        first = true;
    }
    tm->chunks_confirmed = chain.size() - members.size();
    tm->text_bytes = text_n;
    return true;
}

// ---- a gzip file of several members over the ranks of a sharded run (options gzip_in_pieces + gzip_members) -------------------
// The window in front of a part whose text begins `reach[part]` bytes behind the first byte of the member it begins in (clamped
// to 32 768): composed from the out-windows as gzip_compose_windows does - they are the TEXT's tail, whatever members it is made
// of - and then masked: entries more than reach[part] in front of the part are nothing, a marker of that member has no
// business there.  *before = the byte in front of the part's text from the UNMASKED window (whether the part's first byte
// starts a line is a question about the text: lines straddle members), -1 where the file's text begins with the part.
// *valid = false: what gzip_compose_windows refuses, or - for this part or one in front of it - an entry within reach that is
// no byte (a member cannot have begun that far back where the text has not).
// (The window of every part in front is composed again to check its reach: `part` + 1 compositions of 32 768 entries, O(P^2) over
// the ranks of a run - a few ms at the rank counts a node has; a run of hundreds of ranks would keep the windows it has walked.)
inline void gzip_compose_windows_masked(const uint16_t* out_windows, const uint64_t* reach, uint32_t part, uint16_t* in_window, int* before,
                                        bool* valid) {
    std::vector<uint16_t> w(kGzipWindow);
    bool ok = true;
    for (uint32_t r = 0; r <= part; ++r) {
        bool v = false;
        if (r < part && reach[r] == 0) continue;                                // (nothing to check in front of that part)
        gzip_compose_windows(out_windows, r, w.data(), &v);
        if (r == part) ok = ok && v;
        const uint32_t keep = (uint32_t)std::min<uint64_t>(reach[r], kGzipWindow);
        for (uint32_t i = kGzipWindow - keep; i < kGzipWindow; ++i) ok = ok && w[i] < 0x100;
    }
    *before = w[kGzipWindow - 1] < 0x100 ? (int)w[kGzipWindow - 1] : -1;
    const uint32_t keep = (uint32_t)std::min<uint64_t>(reach[part], kGzipWindow);
    for (uint32_t i = 0; i < kGzipWindow; ++i) in_window[i] = i < kGzipWindow - keep ? kGzipNothing : w[i];
    *valid = ok;
}

// What part [a, b) of the text owes the proof of the members that are not its own alone: head_n bytes at a that belong to a
// member begun in front of a (member *head_m), tail_n bytes up to b that belong to a member begun in [a, b) that goes on
// behind b (member *tail_m).  A part that lies inside one member gives its whole text as the head.
inline void gzip_part_owes(const GzipMember* members, uint64_t n_members, uint64_t a, uint64_t b, uint64_t* head_n, uint64_t* head_m, uint64_t* tail_n,
                           uint64_t* tail_m) {
    *head_n = *tail_n = 0;
    *head_m = *tail_m = n_members;
    for (uint64_t m = 0; m < n_members && a < b; ++m) {
        const uint64_t lo = members[m].text_off, hi = lo + members[m].text_n;
        if (lo < a && a < hi) { *head_n = std::min(b, hi) - a; *head_m = m; }
        if (lo >= a && lo < b && b < hi) { *tail_n = b - lo; *tail_m = m; }
    }
}

// Every member proven over the parts.  Part p holds the text [part_a[p], part_b[p]) - the parts in order, back to back from 0
// to the text's end - and gives: local_bad[p], the first member that lies inside its text alone and whose CRC32 is not its
// trailer's (~0: none); {head_reg, head_len} and {tail_reg, tail_len}, the CRC registers (from zero, no final inversion:
// rala_hip_crc32_chain's convention) of what gzip_part_owes names, zeros where it names nothing.  A member that spans parts is
// the chain of the tail of the part it begins in, the heads of the parts behind it, in part order, against ITS trailer; an
// empty member's CRC32 is 0.  crc_chain: kernels.h's gzip_crc_chain.  false with *bad = the first member that fails (n_members: the parts are not the text's).
inline bool gzip_members_proof(const GzipMember* members, uint64_t n_members, const uint64_t* part_a, const uint64_t* part_b, const uint32_t* head_reg,
                               const uint64_t* head_len, const uint32_t* tail_reg, const uint64_t* tail_len, const uint64_t* local_bad, uint32_t parts,
                               uint32_t (*crc_chain)(const uint32_t*, const uint64_t*, uint64_t), uint64_t* bad) {
    *bad = n_members;
    uint64_t total = 0;
    for (uint64_t m = 0; m < n_members; ++m) {
        if (members[m].text_off != total) return false;
        total += members[m].text_n;
    }
    if (!parts || !n_members || part_a[0] != 0 || part_b[parts - 1] != total) return false;
    for (uint32_t p = 0; p < parts; ++p) {
        if (part_b[p] < part_a[p] || (p && part_a[p] != part_b[p - 1])) return false;
    }
    uint64_t first = n_members;
    auto fails = [&](uint64_t m) { first = std::min(first, m); };
    std::vector<uint64_t> want_head(parts), want_tail(parts), head_m(parts), tail_m(parts);
    for (uint32_t p = 0; p < parts; ++p) {
        gzip_part_owes(members, n_members, part_a[p], part_b[p], &want_head[p], &head_m[p], &want_tail[p], &tail_m[p]);
        if (local_bad[p] != ~0ull) fails(std::min<uint64_t>(local_bad[p], n_members - 1));
        // a register nobody owes, or one of another length: the member that holds the byte it claims to begin with
        if (head_len[p] != want_head[p] || tail_len[p] != want_tail[p]) {
            uint64_t m = head_len[p] != want_head[p] ? head_m[p] : tail_m[p];
            const uint64_t at = head_len[p] != want_head[p] ? part_a[p] : (part_b[p] ? part_b[p] - 1 : 0);
            for (uint64_t k = 0; m == n_members && k < n_members; ++k) {
                if (members[k].text_n && members[k].text_off <= at && at < members[k].text_off + members[k].text_n) m = k;
            }
            fails(std::min<uint64_t>(m, n_members - 1));
        }
    }
    for (uint64_t m = 0; m < n_members; ++m) {
        const uint64_t lo = members[m].text_off, hi = lo + members[m].text_n;
        if (lo == hi) {
            if (members[m].crc != 0) fails(m);
            continue;
        }
        std::vector<uint32_t> reg;
        std::vector<uint64_t> len;
        bool spans = false;
        for (uint32_t p = 0; p < parts; ++p) {
            if (tail_m[p] == m) { reg.push_back(tail_reg[p]); len.push_back(tail_len[p]); spans = true; }
            if (head_m[p] == m) { reg.push_back(head_reg[p]); len.push_back(head_len[p]); spans = true; }
        }
        if (!spans) continue;                                       // (inside one part: local_bad's)
        uint64_t sum = 0;
        for (uint64_t l : len) sum += l;
        if (sum != hi - lo || crc_chain(reg.data(), len.data(), reg.size()) != members[m].crc) fails(m);
    }
    *bad = first;
    return first == n_members;
}

}  // namespace ingest
}  // namespace rala_hip
