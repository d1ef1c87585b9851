// C surface of the overlap readers for the CPU test-suite (tests/test_ingest_cpu.py): the
// multi-threaded PAF reader against the line-by-line one; and of the sequence readers (tests/test_sequences_cpu.py,
// tests/test_gpu_sequences.py): what read_fasta / read_fastq give, and the second pass's slicer.  Not part of the product boundary.
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include <string>
#include <unordered_map>
#include <vector>

#include "io.hpp"

namespace {

// FNV-1a-64
uint64_t hash_of(const std::string& s) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned char c : s) h = (h ^ c) * 0x100000001b3ull;
    return h;
}

struct Sequences {
    std::string names;                  // one behind the other
    std::vector<uint32_t> name_len, length;
    std::vector<uint64_t> hash;         // of each read's bases
    bool ok = false;
};

struct Parsed {
    rala::io::OverlapColumns cols;
    int64_t length_error = -1;
    bool ok = false;
};

}  // namespace

extern "C" {

// names: n_reads names separated by '\n'.  parallel = 0: io::read_paf + std::unordered_map (the line-by-line
// reader), 1: io::read_paf_parallel, 2: io::read_overlaps_streamed (PAF, plain or gzip), 3: the same for
// MHAP, 4: io::read_mhap line by line
void* io_paf_parse(const char* path, const char* names, const uint32_t* read_len, uint64_t n_reads, int check_lengths,
                   uint32_t threads, int parallel) {
    std::vector<std::string> nm;
    const char* p = names;
    for (uint64_t i = 0; i < n_reads; ++i) {
        const char* e = strchr(p, '\n');
        nm.emplace_back(p, e ? (size_t)(e - p) : strlen(p));
        p = e ? e + 1 : p + strlen(p);
    }
    std::vector<uint32_t> len(read_len, read_len + n_reads);
    auto* out = new Parsed();
    if (parallel == 1 || parallel == 2 || parallel == 3) {
        rala::io::NameTable table;
        table.build(nm);
        if (parallel == 1) out->ok = rala::io::read_paf_parallel(path, table, len, check_lengths != 0, threads, out->cols, &out->length_error);
        else out->ok = rala::io::read_overlaps_streamed(path, parallel == 3, table, len, check_lengths != 0, threads, out->cols, &out->length_error);
        return out;
    }
    if (parallel == 4) {
        auto& c = out->cols;
        out->ok = rala::io::read_mhap(path, [&](const rala::io::MhapRecord& r) {
            const uint64_t a = r.a_id - 1, b = r.b_id - 1;
            const uint32_t ia = a < len.size() ? (uint32_t)a : 0xFFFFFFFFu, ib = b < len.size() ? (uint32_t)b : 0xFFFFFFFFu;
            if (out->length_error < 0) {
                if (check_lengths && ia != 0xFFFFFFFFu && r.a_length != len[ia]) out->length_error = ia;
                else if (check_lengths && ia != 0xFFFFFFFFu && ib != 0xFFFFFFFFu && r.b_length != len[ib]) out->length_error = ib;
            }
            c.a_id.push_back(ia); c.b_id.push_back(ib);
            c.a_begin.push_back(r.a_begin); c.a_end.push_back(r.a_end);
            c.b_begin.push_back(r.b_begin); c.b_end.push_back(r.b_end);
            c.length.push_back(std::max(r.a_end - r.a_begin, r.b_end - r.b_begin)); c.strand.push_back(r.a_rc == r.b_rc ? 0 : 1);
        });
        return out;
    }
    std::unordered_map<std::string, uint64_t> map;
    for (uint64_t i = 0; i < n_reads; ++i) map[nm[i]] = i;
    auto& c = out->cols;
    out->ok = rala::io::read_paf(path, [&](const rala::io::PafRecord& r) {
        auto a = map.find(r.q_name), b = map.find(r.t_name);
        const uint32_t ia = a == map.end() ? 0xFFFFFFFFu : (uint32_t)a->second;
        const uint32_t ib = b == map.end() ? 0xFFFFFFFFu : (uint32_t)b->second;
        if (out->length_error < 0) {
            if (check_lengths && ia != 0xFFFFFFFFu && r.q_length != len[ia]) out->length_error = ia;
            else if (check_lengths && ia != 0xFFFFFFFFu && ib != 0xFFFFFFFFu && r.t_length != len[ib]) out->length_error = ib;
        }
        c.a_id.push_back(ia); c.b_id.push_back(ib);
        c.a_begin.push_back(r.q_begin); c.a_end.push_back(r.q_end);
        c.b_begin.push_back(r.t_begin); c.b_end.push_back(r.t_end);
        c.length.push_back(r.overlap_length); c.strand.push_back(r.orientation == '+' ? 0 : 1);
    });
    return out;
}

int io_paf_ok(void* h) { return ((Parsed*)h)->ok; }
uint64_t io_paf_size(void* h) { return ((Parsed*)h)->cols.size(); }
int64_t io_paf_length_error(void* h) { return ((Parsed*)h)->length_error; }
void io_paf_copy(void* h, uint32_t* a_id, uint32_t* b_id, uint32_t* a_begin, uint32_t* a_end, uint32_t* b_begin,
                 uint32_t* b_end, uint32_t* length, uint8_t* strand) {
    const auto& c = ((Parsed*)h)->cols;
    const size_t n = c.size();
    memcpy(a_id, c.a_id.data(), n * 4); memcpy(b_id, c.b_id.data(), n * 4);
    memcpy(a_begin, c.a_begin.data(), n * 4); memcpy(a_end, c.a_end.data(), n * 4);
    memcpy(b_begin, c.b_begin.data(), n * 4); memcpy(b_end, c.b_end.data(), n * 4);
    memcpy(length, c.length.data(), n * 4); memcpy(strand, c.strand.data(), n);
}
void io_paf_free(void* h) { delete (Parsed*)h; }

// rala::io::NameTable by itself (tests/test_name_table_cpu.py, tests/test_gpu_name_table.py): built from n names given in order
// (names: one behind the other, name_len their lengths), or adopted from finished buckets; find; the buckets and the arena
// (order: null, or the permutation of the ids in which the names are inserted)
void* io_names_build(const char* names, const uint32_t* name_len, uint64_t n, const uint64_t* order) {
    std::vector<std::string> nm;
    nm.reserve(n);
    for (uint64_t i = 0; i < n; ++i) { nm.emplace_back(names, name_len[i]); names += name_len[i]; }
    auto* t = new rala::io::NameTable();
    t->build(nm, order);
    return t;
}
void* io_names_adopt(const void* buckets, uint64_t n_buckets, const char* arena, uint64_t arena_bytes) {
    auto* t = new rala::io::NameTable();
    t->adopt((const rala_hip::NameBucket*)buckets, n_buckets, std::string(arena ? arena : "", arena ? arena_bytes : 0));
    return t;
}
// What Graph::index_sequences and Graph::initialize do on the host between the device's index and the first tokeniser launch when
// the device does not build the table (tools/name_table_bench.py: the leg to beat): one string per read and its entry in an
// unordered_map, then NameTable::build over the strings.  *map_size: the distinct names (and keeps the map from being optimised away)
void* io_names_strings_map_build(const char* arena, const uint64_t* name_off, const uint32_t* name_len, uint64_t n, uint64_t* map_size) {
    std::vector<std::string> names;
    std::unordered_map<std::string, uint64_t> name_to_id;
    names.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        names.emplace_back(arena + name_off[i], name_len[i]);
        name_to_id[names.back()] = i;
    }
    if (map_size) *map_size = name_to_id.size();
    auto* t = new rala::io::NameTable();
    t->build(names);
    return t;
}
const void* io_names_bucket_ptr(void* h) { return ((rala::io::NameTable*)h)->buckets(); }
const char* io_names_arena_ptr(void* h) { return ((rala::io::NameTable*)h)->arena().data(); }
uint64_t io_names_buckets(void* h) { return ((rala::io::NameTable*)h)->n_buckets(); }
uint64_t io_names_arena_bytes(void* h) { return ((rala::io::NameTable*)h)->arena().size(); }
void io_names_copy(void* h, void* buckets, char* arena) {
    const auto& t = *(rala::io::NameTable*)h;
    if (buckets) memcpy(buckets, (const void*)t.buckets(), t.n_buckets() * sizeof(rala_hip::NameBucket));
    if (arena) memcpy(arena, t.arena().data(), t.arena().size());
}
// the ids of n queries (one behind the other), ~0 where a name is absent
void io_names_find(void* h, const char* queries, const uint32_t* query_len, uint64_t n, uint64_t* id) {
    const auto& t = *(rala::io::NameTable*)h;
    for (uint64_t i = 0; i < n; ++i) { id[i] = t.find(queries, query_len[i]); queries += query_len[i]; }
}
uint64_t io_names_hash(const char* p, uint64_t n) { return rala::io::NameTable::hash(p, n); }
void io_names_free(void* h) { delete (rala::io::NameTable*)h; }

// io::read_fasta (fastq = 0) / io::read_fastq (1): per record the name, the number of bases and a hash of them
void* io_seq_parse(const char* path, int fastq) {
    auto* out = new Sequences();
    auto sink = [&](const std::string& name, const std::string& data) {
        out->names += name;
        out->name_len.push_back((uint32_t)name.size());
        out->length.push_back((uint32_t)data.size());
        out->hash.push_back(hash_of(data));
    };
    out->ok = fastq ? rala::io::read_fastq(path, sink) : rala::io::read_fasta(path, sink);
    return out;
}
int io_seq_ok(void* h) { return ((Sequences*)h)->ok; }
uint64_t io_seq_size(void* h) { return ((Sequences*)h)->length.size(); }
uint64_t io_seq_name_bytes(void* h) { return ((Sequences*)h)->names.size(); }
void io_seq_copy(void* h, char* names, uint32_t* name_len, uint32_t* length, uint64_t* hash) {
    const auto& q = *(Sequences*)h;
    memcpy(names, q.names.data(), q.names.size());
    memcpy(name_len, q.name_len.data(), q.name_len.size() * 4);
    memcpy(length, q.length.data(), q.length.size() * 4);
    memcpy(hash, q.hash.data(), q.hash.size() * 8);
}
void io_seq_free(void* h) { delete (Sequences*)h; }

// io::slice_sequences with an index of n records (n_members BGZF members, 0: a plain file): the hash and the number of
// bases of every wanted read; 1 = ok
int io_seq_slice(const char* path, uint64_t n, const uint64_t* data_off, const uint64_t* data_span, const uint32_t* length,
                 uint64_t n_members, const uint64_t* member_off, const uint32_t* member_bytes, const uint32_t* member_text_bytes,
                 const uint64_t* member_text_off, const uint64_t* wanted, uint64_t n_wanted, uint32_t threads, uint64_t* hash,
                 uint32_t* bases) {
    rala::io::SequenceIndex ix;
    ix.data_off.assign(data_off, data_off + n);
    ix.data_span.assign(data_span, data_span + n);
    ix.length.assign(length, length + n);
    if (n_members) {
        ix.member_off.assign(member_off, member_off + n_members);
        ix.member_bytes.assign(member_bytes, member_bytes + n_members);
        ix.member_text_bytes.assign(member_text_bytes, member_text_bytes + n_members);
        ix.member_text_off.assign(member_text_off, member_text_off + n_members);
    }
    std::vector<std::string> out;
    if (!rala::io::slice_sequences(path, ix, std::vector<uint64_t>(wanted, wanted + n_wanted), threads, out)) return 0;
    for (uint64_t k = 0; k < n_wanted; ++k) {
        hash[k] = hash_of(out[k]);
        bases[k] = (uint32_t)out[k].size();
    }
    return 1;
}

}  // extern "C"
