/*!
 * @file host_api_capi.cpp
 *
 * @brief C entry points over stand-alone rala::Pile / rala::Overlap objects, for the tests that
 * drive the class interface the way the reference's Graph::initialize does (createPile,
 * add_layers, find_valid_region, find_median, find_chimeric_hills, find_chimeric_pits,
 * break_over_*, Overlap::transmute / trim / type; reference src/pile.hpp:19-170,
 * src/overlap.hpp:27-117).  Built into rala_amd/host/librala_api.so; not part of librala.so.
 */

#include <stdio.h>
#include <string.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "io.hpp"
#include "overlap.hpp"
#include "pile.hpp"
#include "sequence.hpp"
#include "rala_hip.h"

namespace {

struct Handle {
    std::vector<std::unique_ptr<rala::Pile>> piles;
    std::unordered_map<std::string, uint64_t> name_to_id;
    std::vector<uint32_t> length;
};

std::string read_name(uint64_t r) { return "read_" + std::to_string(r); }

}  // namespace

extern "C" {

void* hp_create(const uint32_t* read_len, uint64_t n) {
    Handle* h = new Handle();
    for (uint64_t r = 0; r < n; ++r) {
        h->piles.emplace_back(rala::createPile(r, read_len[r]));
        h->name_to_id[read_name(r)] = r;
        h->length.push_back(read_len[r]);
    }
    return h;
}

void hp_destroy(void* p) { delete (Handle*)p; }

void hp_add_layers(void* p, uint64_t r, const uint32_t* bounds, uint64_t n) {
    std::vector<uint32_t> b(bounds, bounds + n);
    ((Handle*)p)->piles[r]->add_layers(b);
}

int hp_find_valid_region(void* p, uint64_t r) { return ((Handle*)p)->piles[r]->find_valid_region() ? 1 : 0; }
void hp_find_median(void* p, uint64_t r) { ((Handle*)p)->piles[r]->find_median(); }
void hp_find_chimeric_hills(void* p, uint64_t r) { ((Handle*)p)->piles[r]->find_chimeric_hills(); }
void hp_find_chimeric_pits(void* p, uint64_t r) { ((Handle*)p)->piles[r]->find_chimeric_pits(); }
int hp_break_over_chimeric_pits(void* p, uint64_t r, uint16_t median) {
    return ((Handle*)p)->piles[r]->break_over_chimeric_pits(median) ? 1 : 0;
}
int hp_break_over_chimeric_hills(void* p, uint64_t r) {
    return ((Handle*)p)->piles[r]->break_over_chimeric_hills() ? 1 : 0;
}
int hp_shrink(void* p, uint64_t r, uint32_t begin, uint32_t end) {
    return ((Handle*)p)->piles[r]->shrink(begin, end) ? 1 : 0;
}
void hp_find_repetitive_hills(void* p, uint64_t r, uint16_t median) { ((Handle*)p)->piles[r]->find_repetitive_hills(median); }
int hp_has_repetitive_hills(void* p, uint64_t r) { return ((Handle*)p)->piles[r]->has_repetitive_hills() ? 1 : 0; }
/*! @brief Pile::to_json; returns the length, copies at most cap bytes */
uint64_t hp_to_json(void* p, uint64_t r, char* out, uint64_t cap) {
    const auto& pile = ((Handle*)p)->piles[r];
    if (pile == nullptr) return 0;
    const std::string s = pile->to_json();
    if (out) memcpy(out, s.data(), s.size() < cap ? s.size() : cap);
    return s.size();
}
/*! @brief Graph::initialize drops a pile whose valid region is too short (graph.cpp:396-399) */
void hp_reset(void* p, uint64_t r) { ((Handle*)p)->piles[r].reset(); }

/*! @brief out = {alive, begin, end, median, p10, has_chimeric_pit, has_chimeric_hill} */
void hp_get(void* p, uint64_t r, uint32_t* out) {
    const auto& pile = ((Handle*)p)->piles[r];
    for (int i = 0; i < 7; ++i) out[i] = 0;
    if (pile == nullptr) return;
    out[0] = 1; out[1] = pile->begin(); out[2] = pile->end(); out[3] = pile->median(); out[4] = pile->p10();
    out[5] = pile->has_chimeric_pit(); out[6] = pile->has_chimeric_hill();
}

uint64_t hp_data(void* p, uint64_t r, uint16_t* out) {
    const auto& pile = ((Handle*)p)->piles[r];
    if (pile == nullptr) return 0;
    const std::vector<uint16_t>& d = pile->data();
    for (size_t i = 0; i < d.size(); ++i) out[i] = d[i];
    return d.size();
}

/*!
 * @brief one PAF record against the current piles: createOverlap, transmute, trim, type.
 * coords = {a_begin, a_end, b_begin, b_end, length} in / out.  Returns 0 when transmute or
 * trim drops the overlap.
 */
int hp_overlap_trim_type(void* p, uint32_t a, uint32_t b, uint32_t strand, uint32_t* coords, int* type_out) {
    Handle* h = (Handle*)p;
    auto o = rala::createOverlap(read_name(a), h->length[a], coords[0], coords[1], strand ? '-' : '+',
        read_name(b), h->length[b], coords[2], coords[3], coords[4]);
    if (!o->transmute(h->piles, h->name_to_id)) return 0;
    if (o->a_id() != a || o->b_id() != b || o->orientation() != strand) return -1;
    if (!o->trim(h->piles)) return 0;
    coords[0] = o->a_begin(); coords[1] = o->a_end(); coords[2] = o->b_begin(); coords[3] = o->b_end();
    coords[4] = o->length();
    *type_out = (int)o->type(h->piles);
    return 1;
}

/*! @brief an MHAP record (1-based ids): the fields createOverlap derives */
int hp_overlap_from_mhap(uint64_t a_id, uint64_t b_id, uint32_t a_rc, uint32_t a_begin, uint32_t a_end,
    uint32_t a_length, uint32_t b_rc, uint32_t b_begin, uint32_t b_end, uint32_t b_length, uint32_t* out) {
    auto o = rala::createOverlap(a_id, b_id, a_rc, a_begin, a_end, a_length, b_rc, b_begin, b_end, b_length);
    out[0] = o->a_id(); out[1] = o->b_id(); out[2] = o->length(); out[3] = o->orientation();
    return 0;
}

// ---- the device tokeniser (rala_hip_set_overlaps_from_paf) for tests/test_gpu_ingest.py: the columns it leaves, to be
// compared with the host readers' (libassembly_graph.so: io_paf_parse).  names: n_reads names separated by '\n'.
struct PafOnDevice {
    int rc = 0, irregular = 0;
    int64_t bad = -1;
    uint64_t n = 0;
    std::vector<uint32_t> col[7];
    std::vector<uint8_t> strand;
    rala_hip_ingest_timings tm = {};
    rala_hip_gzip_timings gz = {};
    std::vector<uint64_t> member_off, member_n;     // rala_hip_get_gzip_members of the call
    std::vector<rala_hip_gzip_pieces_info> pieces;   // rala_hip_get_gzip_pieces_info of every rank (hp_text_device_ranks)
    std::vector<uint32_t> member_crc;
    // rala_hip_get_gzip_members and rala_hip_get_gzip_member_pieces_info of every rank's slice context (hp_text_device_ranks)
    std::vector<std::vector<uint64_t>> rank_member_off, rank_member_n;
    std::vector<std::vector<uint32_t>> rank_member_crc;
    std::vector<rala_hip_gzip_member_pieces_info> member_pieces;
    std::vector<int> before_rc;     // what every rank's call on the file ingested first returned (hp_text_device_ranks)
    int before_irregular = 0;       // what the file ingested first on the same context gave (hp_text_device_after)
    int64_t before_bad = -1;
};

static void* text_on_device(const char* path, const char* names, const uint32_t* read_len, uint64_t n_reads, int check_lengths, uint32_t threads, bool mhap,
                            const char* const* keys = nullptr, const int64_t* values = nullptr, uint32_t n_options = 0, const char* before = nullptr);
void* hp_paf_device(const char* path, const char* names, const uint32_t* read_len, uint64_t n_reads, int check_lengths, uint32_t threads) {
    return text_on_device(path, names, read_len, n_reads, check_lengths, threads, false);
}
// (an MHAP file names its reads by number: no name table)
void* hp_mhap_device(const char* path, const uint32_t* read_len, uint64_t n_reads, int check_lengths, uint32_t threads) {
    return text_on_device(path, "", read_len, n_reads, check_lengths, threads, true);
}
// The two with options of the context set first (rala_hip_set_option: n_options keys and values; mhap != 0: an MHAP file, no
// names) - tests/test_gpu_gzip.py; hp_paf_device_gzip_info gives what rala_hip_get_gzip_timings gave.
void* hp_text_device_with(const char* path, const char* names, const uint32_t* read_len, uint64_t n_reads, int check_lengths, uint32_t threads,
                          int mhap, const char* const* keys, const int64_t* values, uint32_t n_options) {
    return text_on_device(path, mhap ? "" : names, read_len, n_reads, check_lengths, threads, mhap != 0, keys, values, n_options);
}
// hp_text_device_with behind the file `before`, ingested on the same context first, whatever comes of it (before[0], [1] =
// its irregular flags and first length-check offender): does a call that gave up leave the context usable?
void* hp_text_device_after(const char* before, const char* path, const char* names, const uint32_t* read_len, uint64_t n_reads, int check_lengths,
                           uint32_t threads, int mhap, const char* const* keys, const int64_t* values, uint32_t n_options) {
    return text_on_device(path, mhap ? "" : names, read_len, n_reads, check_lengths, threads, mhap != 0, keys, values, n_options, before);
}
void hp_paf_device_before(void* h, int64_t* before) {
    before[0] = ((const PafOnDevice*)h)->before_irregular;
    before[1] = ((const PafOnDevice*)h)->before_bad;
}
static void* text_on_device(const char* path, const char* names, const uint32_t* read_len, uint64_t n_reads, int check_lengths, uint32_t threads, bool mhap,
                            const char* const* keys, const int64_t* values, uint32_t n_options, const char* before) {
    std::vector<std::string> nm;
    const char* p = names;
    for (uint64_t i = 0; i < n_reads && !mhap; ++i) {
        const char* e = strchr(p, '\n');
        nm.emplace_back(p, e ? (size_t)(e - p) : strlen(p));
        p = e ? e + 1 : p + strlen(p);
    }
    rala::io::NameTable table;
    if (!mhap) table.build(nm);
    auto* out = new PafOnDevice();
    rala_hip_ctx* ctx = nullptr;
    out->rc = rala_hip_create(0, &ctx);
    if (out->rc != RALA_HIP_OK) return out;
    for (uint32_t k = 0; k < n_options && out->rc == RALA_HIP_OK; ++k) out->rc = rala_hip_set_option(ctx, keys[k], values[k]);
    if (out->rc == RALA_HIP_OK) out->rc = rala_hip_set_reads(ctx, read_len, n_reads);
    if (out->rc == RALA_HIP_OK && !mhap) out->rc = rala_hip_set_name_table(ctx, table.buckets(), table.n_buckets(), table.arena().data(), table.arena().size());
    if (out->rc == RALA_HIP_OK && before) {
        out->rc = mhap ? rala_hip_set_overlaps_from_mhap(ctx, before, check_lengths, threads, &out->before_bad, &out->before_irregular)
                       : rala_hip_set_overlaps_from_paf(ctx, before, check_lengths, threads, &out->before_bad, &out->before_irregular);
    }
    if (out->rc == RALA_HIP_OK) {
        out->rc = mhap ? rala_hip_set_overlaps_from_mhap(ctx, path, check_lengths, threads, &out->bad, &out->irregular)
                       : rala_hip_set_overlaps_from_paf(ctx, path, check_lengths, threads, &out->bad, &out->irregular);
    }
    if (out->rc == RALA_HIP_OK) rala_hip_get_ingest_timings(ctx, &out->tm);
    if (out->rc == RALA_HIP_OK) rala_hip_get_gzip_timings(ctx, &out->gz);
    uint64_t n_members = 0;
    if (out->rc == RALA_HIP_OK) out->rc = rala_hip_get_gzip_members(ctx, &n_members, 0, nullptr, nullptr, nullptr);
    if (out->rc == RALA_HIP_OK && n_members) {
        out->member_off.resize(n_members); out->member_n.resize(n_members); out->member_crc.resize(n_members);
        out->rc = rala_hip_get_gzip_members(ctx, &n_members, n_members, out->member_off.data(), out->member_n.data(), out->member_crc.data());
    }
    if (out->rc == RALA_HIP_OK && !out->irregular && out->bad < 0) {
        out->rc = rala_hip_get_overlap_columns(ctx, &out->n, nullptr, nullptr);
        uint32_t* cols[7];
        for (int k = 0; k < 7; ++k) { out->col[k].resize(out->n); cols[k] = out->col[k].data(); }
        out->strand.resize(out->n);
        if (out->rc == RALA_HIP_OK) out->rc = rala_hip_get_overlap_columns(ctx, &out->n, cols, out->strand.data());
    }
    rala_hip_destroy(ctx);
    return out;
}
// The same over `world` ranks that share device 0 (in-process transport), every rank on a thread of its own: rank k ships and
// tokenises its byte range of the file, the ranks settle the cuts between runs of equal queries and move the rows in front
// of them (rala_hip_mg_set_overlaps_from_paf).  The handle holds the slices' columns back to back (which must be the
// file's records in order); slices[2 k], [2 k + 1] = file position of rank k's first record and its record count.
// sensitive != 0: the ranks' shares of a sensitive file instead (rala_hip_tokenise_sensitive_paf, no collective, no cuts).
void* hp_paf_device_ranks(const char* path, const char* names, const uint32_t* read_len, uint64_t n_reads, int check_lengths, uint32_t threads,
                          uint32_t world, int sensitive, uint64_t* slices) {
    std::vector<std::string> nm;
    const char* p = names;
    for (uint64_t i = 0; i < n_reads; ++i) {
        const char* e = strchr(p, '\n');
        nm.emplace_back(p, e ? (size_t)(e - p) : strlen(p));
        p = e ? e + 1 : p + strlen(p);
    }
    rala::io::NameTable table;
    table.build(nm);
    auto* out = new PafOnDevice();
    void* group = nullptr;
    out->rc = rala_hip_mg_local_group_create(world, &group);
    if (out->rc != RALA_HIP_OK) return out;
    std::vector<rala_hip_mg*> ranks(world, nullptr);
    for (uint32_t k = 0; k < world && out->rc == RALA_HIP_OK; ++k) out->rc = rala_hip_mg_create_contexts(0, k, world, &ranks[k]);
    std::vector<int> rc(world, RALA_HIP_OK), irregular(world, 0);
    std::vector<int64_t> bad(world, -1);
    std::vector<std::vector<uint32_t>> col[7];
    for (auto& c : col) c.resize(world);
    std::vector<std::vector<uint8_t>> strand(world);
    uint64_t file_bytes = 0;
    if (sensitive) {
        FILE* f = fopen(path, "rb");
        if (f) { fseek(f, 0, SEEK_END); file_bytes = (uint64_t)ftell(f); fclose(f); }
    }
    if (out->rc == RALA_HIP_OK) {
        std::vector<std::thread> th;
        for (uint32_t k = 0; k < world; ++k) {
            th.emplace_back([&, k]() {
                rala_hip_mg* mg = ranks[k];
                int r = rala_hip_mg_join(mg, RALA_HIP_COMM_LOCAL, group);
                if (r == RALA_HIP_OK) r = rala_hip_mg_set_reads(mg, read_len, n_reads);
                rala_hip_ctx* cs = rala_hip_mg_context(mg);
                if (r == RALA_HIP_OK) r = rala_hip_set_name_table(cs, table.buckets(), table.n_buckets(), table.arena().data(), table.arena().size());
                uint64_t first = 0, n = 0;
                std::vector<uint32_t> got[7];
                std::vector<uint8_t> got_strand;
                if (sensitive) {
                    rala_hip_overlaps dev = {};
                    if (r == RALA_HIP_OK) r = rala_hip_tokenise_sensitive_paf(cs, path, file_bytes * k / world, file_bytes * (k + 1) / world, threads, &dev, &n, &irregular[k]);
                    if (r == RALA_HIP_OK && !irregular[k]) {
                        // (read back through the context: the columns are plain device memory, adopted as its overlaps)
                        r = rala_hip_set_overlaps(cs, &dev, n, RALA_HIP_MEM_DEVICE);
                        uint32_t* dst[7];
                        for (int c = 0; c < 7; ++c) { got[c].resize(n); dst[c] = got[c].data(); }
                        got_strand.resize(n);
                        uint64_t n2 = 0;
                        if (r == RALA_HIP_OK) r = rala_hip_get_overlap_columns(cs, &n2, dst, got_strand.data());
                    }
                } else {
                    if (r == RALA_HIP_OK) r = rala_hip_mg_set_overlaps_from_paf(mg, path, check_lengths, threads, &bad[k], &irregular[k]);
                    if (r == RALA_HIP_OK && !irregular[k] && bad[k] < 0) {
                        r = rala_hip_mg_get_slice(mg, &first, &n);
                        uint32_t* dst[7];
                        for (int c = 0; c < 7; ++c) { got[c].resize(n); dst[c] = got[c].data(); }
                        got_strand.resize(n);
                        uint64_t n2 = 0;
                        if (r == RALA_HIP_OK) r = rala_hip_get_overlap_columns(cs, &n2, dst, got_strand.data());
                        if (r == RALA_HIP_OK && n2 != n) r = RALA_HIP_EDEVICE;
                    }
                }
                slices[2 * k] = first; slices[2 * k + 1] = n;
                for (int c = 0; c < 7; ++c) col[c][k] = std::move(got[c]);
                strand[k] = std::move(got_strand);
                rc[k] = r;
            });
        }
        for (auto& t : th) t.join();
    }
    for (uint32_t k = 0; k < world; ++k) {
        if (rc[k] != RALA_HIP_OK && out->rc == RALA_HIP_OK) { out->rc = rc[k]; fprintf(stderr, "[hp_paf_device_ranks] rank %u: %s\n", k, rala_hip_mg_last_error(ranks[k])); }
        out->irregular |= irregular[k];
        if (bad[k] >= 0 && out->bad < 0) out->bad = bad[k];
        for (int c = 0; c < 7; ++c) out->col[c].insert(out->col[c].end(), col[c][k].begin(), col[c][k].end());
        out->strand.insert(out->strand.end(), strand[k].begin(), strand[k].end());
    }
    out->n = out->strand.size();
    for (rala_hip_mg* r : ranks) if (r) rala_hip_mg_destroy(r);
    rala_hip_mg_local_group_destroy(group);
    return out;
}
// hp_paf_device_ranks for a file of either format (mhap != 0: MHAP, no names) and any kind, with options of every rank's slice
// context set first (rala_hip_set_option on rala_hip_mg_context: "bgzf_in_pieces", "gzip_on_device", ...) -
// tests/test_gpu_ranks_compressed.py, tools/ranks_compressed_bench.py.  before != null: the same group ingests that file
// first, whatever comes of it (hp_paf_device_before: its irregular flags and length error) - does a refusal leave the group
// usable?  sensitive != 0: rank k's share of a sensitive file instead (rala_hip_tokenise_sensitive, part k of world; no
// collective) - the pieces joined behind the threads as a caller has to (rala_hip_bgzf_pieces_chain; irregular |= 8 where
// they are not one chain); pieces[3 k ..] = begin, end, empty of rank k's share.
void* hp_text_device_ranks(const char* path, const char* before, const char* names, const uint32_t* read_len, uint64_t n_reads, int check_lengths,
                           uint32_t threads, uint32_t world, int mhap, int sensitive, const char* const* keys, const int64_t* values,
                           uint32_t n_options, uint64_t* slices, uint64_t* pieces) {
    std::vector<std::string> nm;
    const char* p = names;
    for (uint64_t i = 0; i < n_reads && !mhap; ++i) {
        const char* e = strchr(p, '\n');
        nm.emplace_back(p, e ? (size_t)(e - p) : strlen(p));
        p = e ? e + 1 : p + strlen(p);
    }
    rala::io::NameTable table;
    if (!mhap) table.build(nm);
    auto* out = new PafOnDevice();
    void* group = nullptr;
    out->rc = rala_hip_mg_local_group_create(world, &group);
    if (out->rc != RALA_HIP_OK) return out;
    std::vector<rala_hip_mg*> ranks(world, nullptr);
    for (uint32_t k = 0; k < world && out->rc == RALA_HIP_OK; ++k) out->rc = rala_hip_mg_create_contexts(0, k, world, &ranks[k]);
    std::vector<int> rc(world, RALA_HIP_OK), irregular(world, 0), before_irregular(world, 0);
    std::vector<int64_t> bad(world, -1), before_bad(world, -1);
    std::vector<std::vector<uint32_t>> col[7];
    for (auto& c : col) c.resize(world);
    std::vector<std::vector<uint8_t>> strand(world);
    std::vector<uint64_t> share(3 * (size_t)world, 0);
    out->pieces.assign(world, rala_hip_gzip_pieces_info());
    out->member_pieces.assign(world, rala_hip_gzip_member_pieces_info());
    out->before_rc.assign(world, RALA_HIP_OK);
    out->rank_member_off.resize(world); out->rank_member_n.resize(world); out->rank_member_crc.resize(world);
    if (out->rc == RALA_HIP_OK) {
        std::vector<std::thread> th;
        for (uint32_t k = 0; k < world; ++k) {
            th.emplace_back([&, k]() {
                rala_hip_mg* mg = ranks[k];
                int r = rala_hip_mg_join(mg, RALA_HIP_COMM_LOCAL, group);
                if (r == RALA_HIP_OK) r = rala_hip_mg_set_reads(mg, read_len, n_reads);
                rala_hip_ctx* cs = rala_hip_mg_context(mg);
                // (a key "name@k" is rank k's alone and holds for the file ingested `before` only: behind that call rank k takes the
                // group's value of "name", which must be among the keys - ranks that disagree on an option the roll call compares)
                auto own_key = [&](const char* key, std::string* name) {
                    const char* at = strchr(key, '@');
                    if (!at) return false;
                    *name = std::string(key, (size_t)(at - key));
                    return (uint32_t)atoi(at + 1) == k;
                };
                bool disagrees = false;
                for (uint32_t o = 0; o < n_options && r == RALA_HIP_OK; ++o) if (!strchr(keys[o], '@')) r = rala_hip_set_option(cs, keys[o], values[o]);
                for (uint32_t o = 0; o < n_options && r == RALA_HIP_OK; ++o) {
                    std::string name;
                    if (strchr(keys[o], '@')) disagrees = true;
                    if (own_key(keys[o], &name)) r = rala_hip_set_option(cs, name.c_str(), values[o]);
                }
                if (r == RALA_HIP_OK && !mhap) r = rala_hip_set_name_table(cs, table.buckets(), table.n_buckets(), table.arena().data(), table.arena().size());
                uint64_t first = 0, n = 0;
                std::vector<uint32_t> got[7];
                std::vector<uint8_t> got_strand;
                auto read_back = [&](uint64_t rows) {
                    uint32_t* dst[7];
                    for (int c = 0; c < 7; ++c) { got[c].resize(rows); dst[c] = got[c].data(); }
                    got_strand.resize(rows);
                    uint64_t n2 = 0;
                    const int r2 = rala_hip_get_overlap_columns(cs, &n2, dst, got_strand.data());
                    return r2 == RALA_HIP_OK && n2 != rows ? RALA_HIP_EDEVICE : r2;
                };
                if (sensitive) {
                    rala_hip_overlaps dev = {};
                    // (sensitive == 2: through the one collective, rala_hip_mg_tokenise_sensitive - nothing to join behind it)
                    auto take = [&](const char* file, int* irr) {
                        return sensitive == 2 ? rala_hip_mg_tokenise_sensitive(mg, file, mhap ? 1 : 0, threads, &dev, &n, irr)
                                              : rala_hip_tokenise_sensitive(cs, file, mhap ? 1 : 0, k, world, threads, &dev, &n, &share[3 * k], irr);
                    };
                    if (r == RALA_HIP_OK && before) r = take(before, &before_irregular[k]);
                    if (r == RALA_HIP_OK) r = take(path, &irregular[k]);
                    // (read back through the context: the columns are plain device memory, adopted as its overlaps)
                    if (r == RALA_HIP_OK && !irregular[k]) r = rala_hip_set_overlaps(cs, &dev, n, RALA_HIP_MEM_DEVICE);
                    if (r == RALA_HIP_OK && !irregular[k]) r = read_back(n);
                } else {
                    auto ingest = [&](const char* file, int64_t* b, int* irr) {
                        return mhap ? rala_hip_mg_set_overlaps_from_mhap(mg, file, check_lengths, threads, b, irr)
                                    : rala_hip_mg_set_overlaps_from_paf(mg, file, check_lengths, threads, b, irr);
                    };
                    if (r == RALA_HIP_OK && before) {
                        r = ingest(before, &before_bad[k], &before_irregular[k]);
                        out->before_rc[k] = r;
                        if (disagrees) {
                            // (what every rank's call returned is the result - hp_paf_device_before_rc; the group must still be usable)
                            r = RALA_HIP_OK;
                            for (uint32_t o = 0; o < n_options && r == RALA_HIP_OK; ++o) {
                                std::string name;
                                if (!own_key(keys[o], &name)) continue;
                                for (uint32_t q = 0; q < n_options; ++q) if (name == keys[q]) r = rala_hip_set_option(cs, keys[q], values[q]);
                            }
                        }
                        // (nothing was set by a refusal)
                        if (r == RALA_HIP_OK && before_irregular[k] && rala_hip_mg_get_slice(mg, &first, &n) == RALA_HIP_OK) r = RALA_HIP_EDEVICE;
                        first = n = 0;
                    }
                    if (r == RALA_HIP_OK) r = ingest(path, &bad[k], &irregular[k]);
                    if (r == RALA_HIP_OK && !irregular[k] && bad[k] < 0) {
                        r = rala_hip_mg_get_slice(mg, &first, &n);
                        if (r == RALA_HIP_OK) r = read_back(n);
                    } else if (r == RALA_HIP_OK && rala_hip_mg_get_slice(mg, &first, &n) == RALA_HIP_OK) {
                        r = RALA_HIP_EDEVICE;               // (a refusal that left a slice behind)
                    }
                }
                slices[2 * k] = first; slices[2 * k + 1] = n;
                (void)rala_hip_get_gzip_pieces_info(cs, &out->pieces[k]);
                (void)rala_hip_get_gzip_member_pieces_info(cs, &out->member_pieces[k]);
                uint64_t n_members = 0;
                if (rala_hip_get_gzip_members(cs, &n_members, 0, nullptr, nullptr, nullptr) == RALA_HIP_OK && n_members) {
                    out->rank_member_off[k].resize(n_members); out->rank_member_n[k].resize(n_members); out->rank_member_crc[k].resize(n_members);
                    (void)rala_hip_get_gzip_members(cs, &n_members, n_members, out->rank_member_off[k].data(), out->rank_member_n[k].data(),
                                                    out->rank_member_crc[k].data());
                }
                for (int c = 0; c < 7; ++c) col[c][k] = std::move(got[c]);
                strand[k] = std::move(got_strand);
                rc[k] = r;
            });
        }
        for (auto& t : th) t.join();
    }
    for (uint32_t k = 0; k < world; ++k) {
        if (rc[k] != RALA_HIP_OK && out->rc == RALA_HIP_OK) { out->rc = rc[k]; fprintf(stderr, "[hp_text_device_ranks] rank %u: %s\n", k, rala_hip_mg_last_error(ranks[k])); }
        out->irregular |= irregular[k];
        out->before_irregular |= before_irregular[k];
        if (bad[k] >= 0 && out->bad < 0) out->bad = bad[k];
        if (before_bad[k] >= 0 && out->before_bad < 0) out->before_bad = before_bad[k];
        // (every rank the same verdict: one that differs shows as a value no rank gave)
        if (sensitive != 1 && (irregular[k] != irregular[0] || before_irregular[k] != before_irregular[0])) out->irregular |= 1 << 20;
        for (int c = 0; c < 7; ++c) out->col[c].insert(out->col[c].end(), col[c][k].begin(), col[c][k].end());
        out->strand.insert(out->strand.end(), strand[k].begin(), strand[k].end());
    }
    if (sensitive == 1 && out->rc == RALA_HIP_OK && !out->irregular && rala::io::sniff_compression(path) == 1) {
        std::vector<uint64_t> begin(world), end(world);
        std::vector<int> empty(world);
        for (uint32_t k = 0; k < world; ++k) { begin[k] = share[3 * k]; end[k] = share[3 * k + 1]; empty[k] = (int)share[3 * k + 2]; }
        uint64_t file_bytes = 0;
        FILE* f = fopen(path, "rb");
        if (f) { fseek(f, 0, SEEK_END); file_bytes = (uint64_t)ftell(f); fclose(f); }
        if (!rala_hip_bgzf_pieces_chain(begin.data(), end.data(), empty.data(), world, file_bytes)) out->irregular |= 8;
    }
    for (uint32_t k = 0; pieces && k < 3 * world; ++k) pieces[k] = share[k];
    out->n = out->strand.size();
    for (rala_hip_mg* r : ranks) if (r) rala_hip_mg_destroy(r);
    rala_hip_mg_local_group_destroy(group);
    return out;
}
// info[0 .. 5] = return code, irregular flags, first read with a length mismatch (-1 none), records, ship us, tokenise us
void hp_paf_device_info(void* h, int64_t* info) {
    const auto* o = (const PafOnDevice*)h;
    info[0] = o->rc; info[1] = o->irregular; info[2] = o->bad; info[3] = (int64_t)o->n;
    info[4] = (int64_t)(o->tm.ship_ms * 1000.0f); info[5] = (int64_t)(o->tm.tokenize_ms * 1000.0f);
}
// info[0 .. 9] = find us, decode us, resolve us, compressed bytes, text bytes, chunks, with a candidate, confirmed, refuted,
// the most text bytes of one wave
void hp_paf_device_gzip_info(void* h, int64_t* info) {
    const rala_hip_gzip_timings& g = ((const PafOnDevice*)h)->gz;
    info[0] = (int64_t)(g.find_ms * 1000.0f); info[1] = (int64_t)(g.decode_ms * 1000.0f); info[2] = (int64_t)(g.resolve_ms * 1000.0f);
    info[3] = (int64_t)g.compressed_bytes; info[4] = (int64_t)g.text_bytes; info[5] = (int64_t)g.chunks;
    info[6] = (int64_t)g.chunks_with_candidate; info[7] = (int64_t)g.chunks_confirmed; info[8] = (int64_t)g.chunks_refuted;
    info[9] = (int64_t)g.max_wave_text_bytes;
}
// the members rala_hip_get_gzip_members gave behind the call (tests/test_gpu_gzip_members.py): their number; with cap >= it, each
// one's text offset, text size and CRC32
uint64_t hp_paf_device_gzip_members(void* h, uint64_t cap, uint64_t* text_off, uint64_t* text_n, uint32_t* crc32) {
    const auto* o = (const PafOnDevice*)h;
    const uint64_t n = o->member_off.size();
    for (uint64_t k = 0; k < n && cap >= n; ++k) { text_off[k] = o->member_off[k]; text_n[k] = o->member_n[k]; crc32[k] = o->member_crc[k]; }
    return n;
}
// rank k's piece of a gzip file the ranks took together (hp_text_device_ranks; rala_hip_get_gzip_pieces_info): info[0 .. 7] = own
// chunks, own jobs, halo jobs, own text bytes, window markers, longest chase, compose us, exchange us; 0: no such rank
int hp_paf_device_pieces_info(void* h, uint32_t k, int64_t* info) {
    const auto* o = (const PafOnDevice*)h;
    if (k >= o->pieces.size()) return 0;
    const rala_hip_gzip_pieces_info& p = o->pieces[k];
    info[0] = (int64_t)p.own_chunks; info[1] = (int64_t)p.own_jobs; info[2] = (int64_t)p.halo_jobs; info[3] = (int64_t)p.own_text_bytes;
    info[4] = (int64_t)p.window_markers; info[5] = (int64_t)p.longest_chase;
    info[6] = (int64_t)(p.compose_ms * 1000.0f); info[7] = (int64_t)(p.exchange_ms * 1000.0f);
    return 1;
}
// rank k's view of the members of a gzip file the ranks took together (hp_text_device_ranks; rala_hip_get_gzip_members on its slice
// context): their number; with cap >= it, each one's text offset, text size and CRC32
uint64_t hp_paf_device_rank_members(void* h, uint32_t k, uint64_t cap, uint64_t* text_off, uint64_t* text_n, uint32_t* crc32) {
    const auto* o = (const PafOnDevice*)h;
    if (k >= o->rank_member_off.size()) return 0;
    const uint64_t n = o->rank_member_off[k].size();
    for (uint64_t m = 0; m < n && cap >= n; ++m) { text_off[m] = o->rank_member_off[k][m]; text_n[m] = o->rank_member_n[k][m]; crc32[m] = o->rank_member_crc[k][m]; }
    return n;
}
// ... and what its piece saw of them (rala_hip_get_gzip_member_pieces_info): info[0 .. 5] = own candidates, members begun, member
// ends, registers sent, floor stops, compose us; 0: no such rank
int hp_paf_device_member_pieces_info(void* h, uint32_t k, int64_t* info) {
    const auto* o = (const PafOnDevice*)h;
    if (k >= o->member_pieces.size()) return 0;
    const rala_hip_gzip_member_pieces_info& p = o->member_pieces[k];
    info[0] = (int64_t)p.own_candidates; info[1] = (int64_t)p.members_begun; info[2] = (int64_t)p.member_ends; info[3] = (int64_t)p.registers_sent;
    info[4] = (int64_t)p.floor_stops; info[5] = (int64_t)(p.compose_ms * 1000.0f);
    return 1;
}
// what rank k's call on the file ingested first returned (hp_text_device_ranks with `before`; a rala_hip code, 0: no such rank or OK)
int hp_paf_device_before_rc(void* h, uint32_t k) {
    const auto* o = (const PafOnDevice*)h;
    return k < o->before_rc.size() ? o->before_rc[k] : 0;
}
void hp_paf_device_copy(void* h, uint32_t* a_id, uint32_t* b_id, uint32_t* a_begin, uint32_t* a_end, uint32_t* b_begin, uint32_t* b_end,
                        uint32_t* length, uint8_t* strand) {
    const auto* o = (const PafOnDevice*)h;
    uint32_t* dst[7] = {a_id, b_id, a_begin, a_end, b_begin, b_end, length};
    for (int k = 0; k < 7; ++k) memcpy(dst[k], o->col[k].data(), o->n * 4);
    memcpy(strand, o->strand.data(), o->n);
}
void hp_paf_device_free(void* h) { delete (PafOnDevice*)h; }

// rala::createSequence (reference src/sequence.cpp:12-25): the length of what it made - it leaves the process on an empty name / data
uint64_t hp_sequence_length(const char* name, const char* data) { return rala::createSequence(name, data)->data().size(); }

}  // extern "C"
