// Minimal readers for the formats the reference takes through its (un-vendored)
// bioparser submodule: FASTA / FASTQ sequences, PAF / MHAP overlaps, plain or gzip.
// Names are cut at the first whitespace.
#pragma once

#include <stdint.h>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/name_table.h"

namespace rala {
namespace io {

// name, bases
typedef std::function<void(const std::string&, const std::string&)> SequenceSink;
bool read_fasta(const std::string& path, const SequenceSink& sink);
bool read_fastq(const std::string& path, const SequenceSink& sink);

struct PafRecord {
    std::string q_name, t_name;
    uint32_t q_length, q_begin, q_end, t_length, t_begin, t_end, matching_bases, overlap_length, quality;
    char orientation;
};
struct MhapRecord {
    uint64_t a_id, b_id;
    double error;
    uint32_t minmers, a_rc, a_begin, a_end, a_length, b_rc, b_begin, b_end, b_length;
};
bool read_paf(const std::string& path, const std::function<void(const PafRecord&)>& sink);
bool read_mhap(const std::string& path, const std::function<void(const MhapRecord&)>& sink);

bool has_suffix(const std::string& src, const std::string& suffix);
/*! @brief is a single-member gzip overlap file inflated on the device (rala_hip option "gzip_on_device")?  RALA_DEVICE_GZIP=1 / =0
 * says so, read where the file is opened; without it: no - see README.md, "Compressed overlap files", for what was measured */
bool device_gzip_wanted();
/*! @brief ... and is a gzip file of several members that is not BGZF (cat a.gz b.gz, pigz -i) walked member by member there (rala_hip
 * option "gzip_members") instead of handed to the host reader?  RALA_DEVICE_GZIP=2 says so (and says device_gzip_wanted() as well) */
bool device_gzip_members_wanted();

/*! @brief do the compressed and MHAP files that still go to the host readers take the device ingest: a BGZF .paf.gz / .mhap.gz
 * and a plain .mhap in a run on several GPUs (every rank its piece of the file, rala_hip option "bgzf_in_pieces"), a .paf.gz,
 * .mhap or .mhap.gz given with -s (rala_hip_tokenise_sensitive)?  RALA_DEVICE_COMPRESSED=1 says so; without it: no - unmeasured,
 * see README.md, "Compressed overlap files" */
bool device_compressed_wanted();
/*! @brief ... and, beside all of that, does a gzip file of several members that is not BGZF go over the ranks of a run on several
 * GPUs together where device_gzip_members_wanted() (rala_hip options "gzip_on_device", "gzip_in_pieces" and "gzip_members" on every
 * rank)?  RALA_DEVICE_COMPRESSED=2 says so; =1 leaves such a file to the host reader as before - unmeasured */
bool device_compressed_members_wanted();
/*! @brief does Graph::postprocess lay out all components of a round in one call (rala_hip_layout_batch) instead of one
 * rala_hip_layout per component?  RALA_LAYOUT_BATCH=1 says so; without it: no - the same weights either way; many components
 * gain a lot, one giant component loses 1 %, see README.md, "Layout of all components in one call" */
bool layout_batch_wanted();
/*! @brief in a run on several GPUs, do all ranks lay out the components of a round together, the points shared out by cost
 * (rala_hip_mg_layout_batch_threads), instead of the graph's context alone?  RALA_LAYOUT_RANKS=1 says so; without it, or on one
 * GPU: no - the same weights either way; scaling over real devices is unmeasured, see README.md, "Layout shared by the ranks" */
bool layout_ranks_wanted();
/*! @brief what a file is by its first 18 bytes: 0 text (or unreadable), 1 BGZF (what the host reader's BgzfSource recognises),
 * 2 any other gzip file */
int sniff_compression(const std::string& path);

/*! @brief are the piles' coverage rows resident on the device (rala_hip option "pile_rows")?  RALA_PILE_ROWS=0 says no - a row is
 * then rebuilt from the read's overlap bounds when Pile::data() or the -d output asks for it, and the device holds 2 bytes per base
 * less; read where the devices are opened; without it: yes - see README.md, "Piles without resident rows" */
bool pile_rows_wanted();

/*! @brief is the read file indexed on the device (rala_hip_index_sequences) and its second pass cut out of the file with that
 * index?  RALA_DEVICE_SEQUENCES=1 / =0 says so, read where the file is opened; without it: no - see README.md, "Compressed
 * overlap files", for what was measured */
bool device_sequences_wanted();

/*! @brief with the read file indexed on the device (device_sequences_wanted(), and only where that index succeeded): is the name
 * table built there as well, straight from the index (rala_hip_build_name_table), instead of one string per read, a map and
 * NameTable::build on one host thread?  RALA_DEVICE_NAMES=1 says so, read where the file is opened; without it: no - see README.md,
 * "The name table from the device's index", for what was measured */
bool device_names_wanted();

/*! @brief do the nodes of the assembly graph hold their bases as spans of a table on the device (rala_hip_set_bases /
 * rala_hip_slice_sequences' option "keep_bases") and are unitigs, contigs and GFA segments spelled there at the output
 * (rala_hip_spell), instead of strings that are copied and concatenated on the host?  RALA_DEVICE_CONTIGS=1 says so; without
 * it: no - the same bytes either way, see README.md, "Node bases as spans" */
bool device_contigs_wanted();

// ---- the second pass over the read file, from the device's sequence index ----------------------
// Where every read's bases lie (rala_hip_get_sequence_index): the text [data_off, data_off + data_span) with every newline
// and every carriage return in front of one taken out, `length` bases.  A BGZF file: offsets are offsets into its text, and
// the members' file offsets, sizes (BSIZE + 1), text sizes and text offsets (rala_hip_bgzf_index's arrays) say where that
// text lies; a plain file has none.
struct SequenceIndex {
    std::vector<uint64_t> data_off, data_span;
    std::vector<uint32_t> length;
    std::vector<uint64_t> member_off, member_text_off;
    std::vector<uint32_t> member_bytes, member_text_bytes;
    bool empty() const { return data_off.empty(); }
};
// out[k] = the bases of read wanted[k] (ascending), as read_fasta / read_fastq hand them to their sink: the file is mapped,
// num_threads threads copy the spans - of a BGZF file after inflating the members that cover them, and no others.
// false: the file cannot be mapped, or is not what the index describes.
bool slice_sequences(const std::string& path, const SequenceIndex& index, const std::vector<uint64_t>& wanted, uint32_t num_threads,
    std::vector<std::string>& out);

// ---- one-pass, multi-threaded ingest of an uncompressed PAF file into binary columns -------
// (the reference tokenises every line into a heap Overlap twice,
// src/graph.cpp:328,443)

// read name -> id, looked up straight from the bytes of the file (no std::string per field).
// Open addressing over 32-byte buckets: hash, id, length and the first 16 bytes of the name sit
// in ONE cache line, so a lookup of a name of up to 16 characters is one memory access (a table
// of a million names does not fit any cache: with separate offset / length / arena arrays every
// probe was four dependent misses); longer names confirm against the arena.  prefetch() lets a
// caller start the bucket's load while it parses on (io.cpp: lines are resolved in batches).
class NameTable {
public:
    // order (optional, a permutation of the ids): the names are inserted in this order, names[order[k]] as id order[k] -
    // which slot of its probe path a name takes depends on it, no answer does as long as a name's last id comes last
    void build(const std::vector<std::string>& names, const uint64_t* order = nullptr);
    // takes over a finished table - the one the device built from its sequence index (rala_hip_get_name_table): n_buckets (a
    // power of two) buckets, copied, and the bytes their `off` point into.  The host readers then probe exactly what the device built.
    void adopt(const rala_hip::NameBucket* buckets, size_t n_buckets, std::string arena);
    static uint64_t hash(const char* p, size_t n);
    void prefetch(uint64_t h) const { if (bucket_) __builtin_prefetch(&bucket_[h & mask_]); }
    // id of the name [p, p + n) whose hash is h, or ~0ull
    uint64_t find(const char* p, size_t n, uint64_t h) const;
    uint64_t find(const char* p, size_t n) const { return find(p, n, hash(p, n)); }
    // the table as it is, for the device tokeniser (rala_hip_set_name_table)
    const rala_hip::NameBucket* buckets() const { return bucket_; }
    size_t n_buckets() const { return n_bucket_; }
    const std::string& arena() const { return arena_; }
private:
    typedef rala_hip::NameBucket Bucket;
    // (2 MiB-aligned block marked for transparent huge pages: a probe of a 64 MB table would
    // otherwise miss the TLB as well as the caches)
    Bucket* bucket_ = nullptr;
    size_t n_bucket_ = 0;
    std::string arena_;
    uint64_t mask_ = 0;
public:
    NameTable() = default;
    ~NameTable();
    NameTable(const NameTable&) = delete;
    NameTable& operator=(const NameTable&) = delete;
};

// allocator whose resize() leaves new elements uninitialised (the readers overwrite all of them;
// zero-filling 29 bytes per overlap on one thread would cost as much as parsing)
// Large blocks are 2 MiB aligned and marked for transparent huge pages: a 50 M-overlap file puts
// 6 GB of fresh memory behind these vectors - 1.5 M first-touch faults with 4 KiB pages.
void* allocate_block(size_t bytes);
void free_block(void* p, size_t bytes);

template <class T>
struct UninitAllocator : std::allocator<T> {
    template <class U> struct rebind { typedef UninitAllocator<U> other; };
    UninitAllocator() = default;
    template <class U> UninitAllocator(const UninitAllocator<U>&) {}
    T* allocate(size_t n) { return (T*)allocate_block(n * sizeof(T)); }
    T* allocate(size_t n, const void*) { return allocate(n); }
    void deallocate(T* p, size_t n) { free_block(p, n * sizeof(T)); }
    template <class U> void construct(U* p) { ::new ((void*)p) U; }
    template <class U, class... A> void construct(U* p, A&&... a) { ::new ((void*)p) U(std::forward<A>(a)...); }
};

struct OverlapColumns {
    typedef std::vector<uint32_t, UninitAllocator<uint32_t>> U32;
    typedef std::vector<uint8_t, UninitAllocator<uint8_t>> U8;
    U32 a_id, b_id, a_begin, a_end, b_begin, b_end, length;
    U8 strand;
    size_t size() const { return a_id.size(); }
};

// Appends the records of `path` to `out` in file order.  Ids of unknown names are 0xFFFFFFFF.
// Same checks as Overlap::transmute (src/overlap.cpp:36-82): a PAF length that differs from
// the sequence's is fatal - returned as the offending read id in *length_error (the first such
// line in file order), the caller prints the reference's message.  false = cannot open / map.
bool read_paf_parallel(const std::string& path, const NameTable& names, const std::vector<uint32_t>& read_len,
    bool check_lengths, uint32_t num_threads, OverlapColumns& out, int64_t* length_error);

// The same result for a gzip-compressed (or plain) PAF file, or an MHAP file (mhap = true: blank-separated
// columns, 1-based ids, reference src/overlap.cpp:12-20; `names` is not used then): ONE thread inflates -
// a gzip stream cannot be cut - and hands blocks of whole lines to the others, which parse them with the
// tokenizer of read_paf_parallel.
bool read_overlaps_streamed(const std::string& path, bool mhap, const NameTable& names, const std::vector<uint32_t>& read_len,
    bool check_lengths, uint32_t num_threads, OverlapColumns& out, int64_t* length_error);

}  // namespace io
}  // namespace rala
