// librala_hip context: device arenas + host-side state of one data set.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include <memory>
#include <string>
#include <vector>

#include "geom.h"
#include "host_pool.h"
#include "kernels.h"
#include "rala_hip.h"

namespace rala_hip {

struct HostOvl {
    uint32_t src;        // index in the input overlap arrays
    uint32_t a, b;
    Coords c;
    uint8_t strand;
    uint8_t dead;
    uint8_t type;        // cached Overlap::type, 255 = stale (a pile or the coordinates changed)
};

struct LaunchClass {
    uint32_t lw;         // LDS elements per array
    uint32_t first;      // range in the order array
    uint32_t count;
    bool in_lds;
};

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    // (round 6: the buffer as physical chunks mapped side by side into one reserved range - ensure_chunked; the rows of the piles)
    std::vector<hipMemGenericAllocationHandle_t> chunks;
    std::vector<void*> mapped;          // where chunk i is mapped (null: created, not mapped - a call that failed half way)
    size_t reserved = 0, chunk_size = 0;
    ~DevBuf() { release(); }
    void release() {
        if (reserved) {
            (void)hipDeviceSynchronize();       // (hipFree waits for the device's work by itself; unmapping does not)
            for (size_t i = 0; i < chunks.size(); ++i) {
                if (mapped[i]) (void)hipMemUnmap(mapped[i], chunk_size);
                (void)hipMemRelease(chunks[i]);
            }
            // The RANGE is not given back (hipMemAddressFree): the next reservation would be handed the same addresses, and a
            // kernel of the next context then wrote through translations of the OLD mapping - rows read back as zeros or as another
            // data set's in 3 runs of 8 of tests/test_gpu_parity.py::test_rows_in_mapped_chunks, none in 8 once no address is ever
            // mapped twice.  Address space is what leaks (a context's rows, out of 128 TB); when a reservation fails the caller
            // falls back to hipMalloc.
            chunks.clear();
            mapped.clear();
            reserved = 0;
            chunk_size = 0;
        } else if (p) {
            (void)hipFree(p);
        }
        p = nullptr;
        n = 0;
    }
    // chunk_bytes per physical allocation, mapped in the order of allocation
    // fail_at (tests, option debug_chunk_fail): the mapping fails at chunk fail_at (the caller falls back); negative: never
    hipError_t ensure_chunked(size_t count, size_t chunk_bytes, int device, int64_t fail_at = -1) {
        if (count <= n && p) return hipSuccess;
        release();
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = device;
        size_t gran = 0;
        hipError_t e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
        if (e != hipSuccess) return e;
        if (gran == 0) gran = 2u << 20;
        chunk_bytes = (chunk_bytes + gran - 1) / gran * gran;
        const size_t n_chunks = (count * sizeof(T) + chunk_bytes - 1) / chunk_bytes;
        const size_t bytes = n_chunks * chunk_bytes;
        void* base = nullptr;
        e = hipMemAddressReserve(&base, bytes, 0, nullptr, 0);       // (an alignment asked for here is not honoured: 2 MB whatever)
        if (e != hipSuccess) return e;
        p = (T*)base;
        reserved = bytes;
        chunk_size = chunk_bytes;
        for (size_t i = 0; i < n_chunks && e == hipSuccess; ++i) {
            hipMemGenericAllocationHandle_t h;
            if (fail_at >= 0 && (size_t)fail_at == i) { e = hipErrorOutOfMemory; break; }
            e = hipMemCreate(&h, chunk_bytes, &prop, 0);
            if (e != hipSuccess) break;
            chunks.push_back(h);
            mapped.push_back(nullptr);
            void* at = (char*)base + i * chunk_bytes;
            e = hipMemMap(at, chunk_bytes, 0, h, 0);
            if (e == hipSuccess) mapped.back() = at;
        }
        if (e == hipSuccess) {
            hipMemAccessDesc acc = {};
            acc.location = prop.location;
            acc.flags = hipMemAccessFlagsProtReadWrite;
            e = hipMemSetAccess(base, bytes, &acc, 1);
        }
        if (e != hipSuccess) { release(); return e; }
        n = bytes / sizeof(T);
        return hipSuccess;
    }
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    // Elements [first, first + count) to the host, chunk by chunk (every copy inside ONE of the runtime's allocations).
    hipError_t copy_to_host(void* dst, size_t first, size_t count) const {
        const char* src = (const char*)(p + first);
        size_t left = count * sizeof(T);
        while (left) {
            size_t take = left;
            if (chunk_size) take = std::min(left, chunk_size - (size_t)(src - (const char*)p) % chunk_size);
            const hipError_t e = hipMemcpy(dst, src, take, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return e;
            dst = (char*)dst + take; src += take; left -= take;
        }
        return hipSuccess;
    }
    // room for `count` elements, the first `keep` kept (a blocking copy when the buffer has to move)
    hipError_t grow(size_t keep, size_t count) {
        if (count <= n && p) return hipSuccess;
        T* q = nullptr;
        const size_t want = count + count / 4 + 1;
        hipError_t e = hipMalloc((void**)&q, want * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep && p) e = hipMemcpy(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) { (void)hipFree(q); return e; }
        if (p) (void)hipFree(p);
        p = q;
        n = want;
        return hipSuccess;
    }
};

// pinned host staging buffer (fast, truly asynchronous device <-> host copies)
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t n = 0;
    ~PinnedBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        release();
        if (count == 0) count = 1;
        count += count / 4;                 // grow with slack: survivor counts vary little
        hipError_t e = hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) n = count;
        return e;
    }
};

}  // namespace rala_hip

struct rala_hip_ctx {
    int device = 0;
    uint32_t n_compute_units = 256;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;         // duplicate removal runs here, beside the bucketing
    hipStream_t aux = nullptr;          // the pile chain's small kernels (long and event-dense reads), beside the first one
    bool use_side_stream = true;
    std::string err;
    hipEvent_t ev[12] = {};                // (their names and roles: Event, slots.h)
    // RALA_HIP_MEM_HOST_ASYNC: the columns' host addresses until rala_hip_initialize has uploaded them (copy stream; events:
    // ids, b coordinates, a coordinates, lengths there)
    hipStream_t copy = nullptr;
    hipEvent_t ev_up[4] = {};
    bool upload_pending = false, upload_queued = false;      // queued: every copy of this call's upload is on the copy stream
    const uint32_t* up_src[7] = {};
    const uint8_t* up_strand = nullptr;

    // options
    int64_t pool_per_read_x1000 = 1000;
    int64_t max_lds_read_len = 22000;
    int64_t debug_pile_stop_after = 99;
    int64_t host_threads = 0;                       // 0 = min(hardware threads, 16)
    std::unique_ptr<rala_hip::HostPool> pool;
    bool use_run_kernel = true;
    bool debug_fail_construct = false;          // tests: pass 2 fails on this context
    uint32_t debug_dedupe_list_cap = 0;         // tests: duplicate removal's mark list holds this many marks (0 = 2^20); more: the pass over all overlaps
    uint32_t debug_fp_lds_limit = 0xFFFFFFFFu;  // tests: containment fixed points with more killers than this take the long lists' kernel
    uint32_t debug_fp_give_up = 0;              // tests: the long lists' workgroups do not meet (FixedPointList::debug_give_up: 1 or 2)
    int64_t debug_chunk_fail = -1;              // tests: the mapping of the rows' chunks fails at this chunk (DevBuf::ensure_chunked)
    uint32_t debug_part_shift = 0;              // tests / measurements: BucketTuning::part_shift
    uint32_t debug_count_window = 0;            // tests: BucketTuning::count_window
    bool use_bound_records = true;              // sharded runs: 8-byte bound records instead of two tuples per overlap side where they fit
    bool use_round_batches = true;              // containment fixed point: several rounds per look at the counter
    rala_hip::DevBuf<uint32_t> d_round_log;     // list sizes after the rounds the host did not look at

    // reads
    uint64_t n_reads = 0;
    uint32_t max_read_len = 0;
    // reads by length class (kernels.h: kPileClassBases): each class has its own first kernel in the
    // pile chain.  d_class_order lists the reads class by class; empty when every read is in class 0.
    uint32_t n_class[rala_hip::kPileClasses] = {};
    rala_hip::DevBuf<uint32_t> d_class_order;
    rala_hip::DevBuf<uint32_t> d_seg_base;            // tail: where each segment of the final overlap list ends
    rala_hip::DevBuf<uint32_t> d_dense;               // reads with more events than the first kernels take (+ its counter behind)
    std::vector<uint32_t> h_read_len;
    std::vector<uint64_t> h_pile_off;
    uint64_t pile_elems = 0;
    rala_hip::DevBuf<uint32_t> d_read_len;
    rala_hip::DevBuf<uint64_t> d_pile_off;
    rala_hip::DevBuf<uint16_t> d_pile;
    rala_hip::DevBuf<uint32_t> d_order, d_overflow;
    // reads whose region / interval lists outgrow the position-space kernels' LDS lists: noted in d_big_list[0], run
    // again with the lists in d_big_space at growing sizes (those that still do not fit: the other list)
    rala_hip::DevBuf<uint32_t> d_big_list[2], d_big_space;
    int64_t debug_big_caps = 0;         // tests: first sizes of the lists in global memory (0: the defaults)
    bool debug_force_big = false;       // tests: every read of the position-space kernels runs with its lists in global memory
    rala_hip::DevBuf<uint16_t> d_slab;
    std::vector<rala_hip::LaunchClass> classes;

    // the device tokeniser (ingest.hip): the host's name table as it is, the file's text, the columns it leaves
    rala_hip::DevBuf<uint8_t> d_name_buckets, d_name_arena, d_paf_text, d_paf_strand;
    uint64_t n_name_buckets = 0, n_name_arena_bytes = 0;
    // ... or the table built here from the sequence index (name_table.hip: rala_hip_build_name_table): the insert kernel's words
    // (error, longest probe path, taken buckets), the events around the two kernels, the last build
    rala_hip::DevBuf<uint32_t> d_name_stats;
    hipEvent_t ev_names[2] = {};
    rala_hip_name_table_info name_table_info = {};
    rala_hip::DevBuf<uint32_t> d_paf_col[7], d_paf_chunk[2], d_paf_win[7];
    rala_hip::DevBuf<uint8_t> d_paf_win_strand;
    int64_t ingest_window_bytes = 0;    // option: the tokeniser's window over the file's text (0: a quarter of the free device memory)
    rala_hip::DevBuf<unsigned long long> d_paf_bad;
    rala_hip_ingest_timings ingest_tm = {};
    // BGZF files (ingest_bgzf.hip, inflate_kernels.hip): the compressed bytes, the members' jobs, the inflater's flag
    rala_hip::DevBuf<uint8_t> d_bgzf_comp, d_bgzf_jobs;
    rala_hip::DevBuf<uint32_t> d_bgzf_flag;
    rala_hip_inflate_timings inflate_tm = {};
    // single-member gzip files (option gzip_on_device; ingest_gzip.hip): the chunks' starts and spans, the true
    // chunks' jobs and text offsets, the 16-bit symbols, the segments' CRCs, the resident text
    bool gzip_on_device = false;
    bool gzip_members = false;                  // option: a file of several members is walked member by member (with gzip_on_device)
    bool gzip_in_pieces = false;                // option: the ranks of a sharded run take a single-member gzip overlap file together (with gzip_on_device)
    bool bgzf_in_pieces = false;                // option: a rank of a sharded run takes its piece of a BGZF overlap file (rala_hip_mg_set_overlaps_from_*)
    int64_t gzip_chunk_bytes = 64 << 10;        // option: compressed bytes per chunk
    uint32_t debug_gzip_false_sync = 0;         // tests: every n-th chunk is given a bogus start at its first bit
    rala_hip::DevBuf<uint64_t> d_gzip_starts, d_gzip_off, d_gzip_floor;
    rala_hip::DevBuf<uint8_t> d_gzip_spans, d_gzip_jobs, d_gzip_text;
    rala_hip::DevBuf<uint16_t> d_gzip_sym;
    rala_hip::DevBuf<uint32_t> d_gzip_crc;
    // ... and of a file of several members (option gzip_members): the member find's tile counts, its candidates and their spans,
    // the pieces of the text cut at member ends and their CRC registers; the members of the last call (rala_hip_get_gzip_members)
    rala_hip::DevBuf<uint32_t> d_gzip_tile, d_gzip_piece_crc;
    rala_hip::DevBuf<uint8_t> d_gzip_cands, d_gzip_mspans, d_gzip_pieces;
    std::vector<rala_hip::GzipMember> gzip_members_last;
    rala_hip_gzip_timings gzip_tm = {};
    rala_hip_gzip_pieces_info gzip_pieces = {}; // the rank's piece of the last such ingest (rala_hip_get_gzip_pieces_info)
    rala_hip_gzip_member_pieces_info gzip_member_pieces = {};   // ... of a file of several members (rala_hip_get_gzip_member_pieces_info)
    rala_hip::DevBuf<uint32_t> d_gzip_compose_stats;    // four words of gzip_window_compose_kernel's own
    // the sequence index (ingest_sequences.hip: rala_hip_index_sequences; sequence_kernels.hip): events, records, the names' arena
    int64_t debug_sequence_window = 0;          // tests: the window over the read file's text (0: as the overlap ingest's, 2 GiB at most)
    rala_hip::DevBuf<uint64_t> d_seq_event[2], d_seq_name_pos, d_seq_data_off, d_seq_data_stripped, d_seq_name_off, d_seq_span;
    rala_hip::DevBuf<uint32_t> d_seq_name_len, d_seq_length, d_seq_tile[2], d_seq_name_at, d_seq_flags;
    rala_hip::DevBuf<uint8_t> d_seq_arena;
    uint64_t n_seq_records = 0, n_seq_name_bytes = 0;
    bool seq_index_valid = false;
    rala_hip_ingest_timings seq_tm = {};
    // what the second pass (ingest_sequences.hip: rala_hip_slice_sequences) needs of the index: what it was made from (0 a plain file,
    // 1 BGZF, 2 a single gzip member - then the chain of its true chunks, text offsets from the text's start, and its CRC32),
    // the file's and the text's size, the stripped bytes of the whole text
    int seq_source = 0;
    bool seq_fastq = false;
    uint64_t seq_file_n = 0, seq_text_n = 0, seq_n_stripped = 0;
    std::vector<rala_hip::GzipJob> seq_gzip_chain;
    std::vector<rala_hip::GzipMember> seq_gzip_members;     // (every member's text range, trailer offset and CRC32)
    uint32_t seq_gzip_crc = 0;
    rala_hip::DevBuf<uint16_t> d_gzip_carry;
    rala_hip::DevBuf<uint8_t> d_gzip_hold, d_slice_out;
    rala_hip::DevBuf<uint64_t> d_slice_w[3];
    rala_hip_sequence_slice_info slice_info = {};
    // the table of bases that spans speak of (spell.hip: rala_hip_set_bases, or what rala_hip_slice_sequences gathered with
    // the option keep_bases) - the context's, whatever happens to its reads and piles - and what rala_hip_spell uploads and
    // fills per call: the spans, their output offsets, a window of output
    bool keep_bases = false;                    // option
    uint32_t spell_window_mb = 256;             // option: what a window of spelled bytes may take
    int64_t debug_spell_window = 0;             // tests: the window in bytes (whole tiles, one at least)
    rala_hip::DevBuf<uint8_t> d_bases, d_spell_out;
    rala_hip::DevBuf<uint64_t> d_base_off, d_spell_off;
    rala_hip::DevBuf<rala_hip_span> d_spell_spans;
    std::vector<uint64_t> h_base_off;           // n_base_sources + 1 entries; empty: no table
    uint64_t n_base_sources = 0;
    bool bases_from_slice = false;
    rala_hip_spell_info spell_info = {};

    // overlaps
    uint64_t n_ovl = 0;
    rala_hip::OvlSoA ovl = {};
    rala_hip::DevBuf<uint32_t> d_ovl_u32[7];
    rala_hip::DevBuf<uint8_t> d_ovl_strand;
    rala_hip::DevBuf<uint8_t> d_valid, d_suspect;
    rala_hip::DevBuf<uint32_t> d_dedupe_list;      // where the counting pass marked queries (positions, then queries)
    bool valid_ready = false;
    bool inputs_set = false;            // rala_hip_set_overlaps / _set_bound_tuples was called

    // bound tuples shipped in by the caller instead of overlaps (multi-GPU owners)
    bool tuple_mode = false;
    uint64_t n_tuples = 0;
    const uint2* tuples = nullptr;      // {x = local read, y = bound}
    const uint64_t* records = nullptr;  // bound records instead (rala_hip_set_bound_records): n_records of them
    uint64_t n_records = 0;
    rala_hip::DevBuf<uint64_t> d_record;
    rala_hip::DevBuf<uint2> d_tuple;
    rala_hip::DevBuf<uint32_t> d_owner_cnt;
    bool piles_resident = false;
    // sharded runs, the bounds scattered ONCE on the sender (bucket_kernels.hip, "sharded runs").  A sender: the groups'
    // counts, the partitions' cursors, the blocks' lengths; duplicate removal runs beside the emit on the side stream and is
    // joined by the second pass (dedupe_pending).  An owner: its input is the blocks of all senders as they lie in the
    // runner's buffers (blocks_mode, with tuple_mode).
    bool use_fused_emit = true;
    rala_hip::DevBuf<uint32_t> d_shard_group, d_shard_part, d_shard_words, d_shard_tiles;
    bool dedupe_pending = false;
    bool lists_pending = false;         // a sharded run's survivor lists are being gathered on the side stream (event kEvGatherJoin)
    bool blocks_mode = false;
    const uint64_t* blocks_base = nullptr;
    const uint64_t* blocks_base_self = nullptr;
    rala_hip::ShardBlocks blocks = {};
    rala_hip::ShardGeometry shard_geom = {};
    uint64_t n_block_records = 0;

    // bound CSR
    rala_hip::DevBuf<uint32_t> d_ev_off, d_cursor, d_ev, d_slot_rank[2], d_ev_fixed;
    uint32_t pile_chunk_mb = 1024;      // the rows' buffer as physical chunks of this size (0: one hipMalloc) - initialize.hip
    // Rows on demand (option pile_rows = 0; pile_rows_kernel.hip): initialize allocates no rows and its kernels store none; a row
    // is rebuilt from the read's events - which stay where initialize left them - into d_rows_scratch when somebody asks
    uint32_t pile_rows = 1;             // the option (read by the next rala_hip_initialize)
    uint32_t pile_rows_scratch_mb = 256;        // option: what a batch of rebuilt rows may take (grows to the longest row)
    bool rowless = false;               // how the last rala_hip_initialize ran
    bool sens_csr_ready = false;        // d_sens_off / d_sens_ev hold the bounds of a sensitive construct that SUCCEEDED since the last initialize
    bool sens_pass_running = false;     // ... of the sensitive pass that is under way (its repeat-hill kernels read the rows with them on top)
    uint64_t rows_materialised = 0;     // rows rebuilt since the last initialize
    rala_hip::DevBuf<uint16_t> d_rows_scratch;
    rala_hip::DevBuf<uint64_t> d_rows_off;      // per read: where its row lies in the scratch (valid for the reads of the last batch)
    rala_hip::DevBuf<uint32_t> d_rows_list;
    std::vector<uint64_t> h_rows_off;
    bool debug_ev_events = false;
    uint32_t ev_shift = 0;              // units of d_ev_off: 1 << ev_shift events (kernels.h: kBucketPairShift)
    rala_hip::DevBuf<unsigned char> d_scan_ws;

    // per-read annotation
    rala_hip::DevBuf<uint32_t> d_begin, d_end, d_iv_slot;
    rala_hip::DevBuf<uint16_t> d_median, d_p10;
    rala_hip::DevBuf<uint8_t> d_alive;
    rala_hip::DevBuf<uint32_t> d_n_pits, d_n_hills;
    rala_hip::DevBuf<rala_hip::Interval> d_pool;
    rala_hip::DevBuf<uint32_t> d_small;      // counts and flags of every stage, sixteen words: who owns which, slots.h
    uint32_t pool_cap = 0;
    uint32_t pool_cap_first = 0;        // what set_reads derived from the option
    uint32_t rep_pool_cap = 0;          // repeat hills (sensitive pass); starts at pool_cap_first

    // pass 2
    rala_hip::DevBuf<uint8_t> d_cls;
    rala_hip::DevBuf<uint32_t> d_death[2];
    rala_hip::DevBuf<uint32_t> d_chunk[4];      // survivors per chunk (overlaps, internals) and their scans
    rala_hip::DevBuf<uint4> d_rec;              // packed per-read records of the second pass
    rala_hip::DevBuf<uint8_t> d_crec;           // compact ones (valid region + flags, 4 or 8 bytes per read)
    rala_hip::DevBuf<uint8_t> d_fate;           // per read after the containment scan: never dies | has hills << 1
    rala_hip::DevBuf<uint64_t> d_scan_state;    // tile states of the single-pass scans (scan_pass.h)
    rala_hip::DevBuf<uint32_t> d_counts;        // small device counters of the second pass and the tail (slots.h)
    rala_hip::DevBuf<uint32_t> d_surv_u32[8];
    rala_hip::DevBuf<uint8_t> d_surv_u8[2];
    rala_hip::DevBuf<uint8_t> d_list_block[2];  // sharded runs: this slice's packed survivors / all slices'
    rala_hip::PinnedBuf<uint32_t> p_surv_u32[8];
    rala_hip::PinnedBuf<uint8_t> p_surv_u8[2];

    // host mirror of the per-read state (valid after initialize / construct)
    bool initialized = false, constructed = false;
    uint64_t n_prefiltered = 0;
    std::vector<uint32_t> h_begin, h_end, h_slot;
    std::vector<uint16_t> h_median, h_p10;
    std::vector<uint8_t> h_alive;
    std::vector<uint32_t> h_n_pits, h_n_hills;
    std::vector<rala_hip::Interval> h_pool;
    rala_hip::DevBuf<uint32_t> d_overflow_mid, d_overflow_long, d_chain_cnt;      // more overflow lists / chain counters
    // how initialize left the primary bound events (the sensitive pass reads them again):
    // fixed slots (d_ev_fixed, counts in d_cursor) or the CSR (d_ev_off, d_ev)
    bool ev_ready = false, ev_fixed = false;
    // bounds of the sensitive overlaps by read (CSR), the list of reads of a sensitive-pass launch
    rala_hip::DevBuf<uint32_t> d_sens_off, d_sens_cur, d_sens_ev, d_sens_list, d_sens_split;
    rala_hip::DevBuf<double> d_layout[4];
    rala_hip::DevBuf<uint32_t> d_layout_adj[2];
    // rala_hip_layout_batch (layout.hip): what one call uploads, packed (positions, k, offsets, lists, tiles), the second
    // position buffers behind it; the host side of the one copy each way; the events around the device work
    rala_hip::DevBuf<unsigned char> d_layout_batch;
    rala_hip::PinnedBuf<unsigned char> p_layout_batch;
    hipEvent_t ev_layout[2] = {};
    int64_t layout_fused_max = 1024;      // option: components of at most this many points run fused (0: none)
    rala_hip_layout_info layout_info = {};
    // pinned staging of small device -> host reads (context.hip: d2h_small / stream_sync)
    struct StagedCopy { void* dst; size_t offset, bytes; };
    rala_hip::PinnedBuf<uint32_t> p_stage;
    std::vector<StagedCopy> stage_pending;
    size_t stage_used = 0;
    int64_t use_fixed_buckets = 1;        // single-pass bucketing into fixed slots when they fit
    bool use_partitioned_buckets = true;  // target side through partitioning passes (bucket_kernels.hip) where the input suits
    rala_hip::DevBuf<uint32_t> d_bk_u32[3], d_bk_part, d_bk_group, d_bk_tiles;     // per-read counts; partition / group bases; level-2 tiles
    rala_hip::DevBuf<uint64_t> d_bk_rec[2];                            // target records after level 1 / level 2
    bool host_state_fresh = false;      // host mirrors of the per-read state match the device
    uint32_t pool_used = 0;             // interval pool records in use

    // sensitive pass (repeat hills)
    rala_hip::DevBuf<uint16_t> d_dataset_median;
    rala_hip::DevBuf<uint32_t> d_n_rep;
    // sensitive overlaps on the device: columns, transmuted target side, trimmed coordinates, tuples
    rala_hip::DevBuf<uint32_t> d_sens_col[7], d_sens_tb[2], d_sens_c[5];
    rala_hip::DevBuf<uint2> d_sens_tuples, d_sens_part, d_sens_recv;
    rala_hip::DevBuf<uint64_t> d_sens_rec;     // one context: the target bounds as 8-byte records     // as emitted / grouped by owner / received
    rala_hip::DevBuf<uint8_t> d_gather[2];     // sharded runs: this rank's block / all ranks' blocks of a gather
    rala_hip::DevBuf<uint8_t> d_sens_strand, d_sens_state;
    bool sens_in_device = false;        // option "sensitive_in_device_memory"
    rala_hip::DevBuf<uint32_t> d_rep_slot;
    rala_hip::DevBuf<rala_hip::Interval> d_rep_pool;
    std::vector<uint32_t> h_n_rep;
    std::vector<uint32_t> h_rep_slot;
    std::vector<rala_hip::Interval> h_rep_pool;
    bool have_repeats = false;
    bool rep_host_stale = false;        // the hills are on the device, the host vectors above not yet fetched
    uint32_t n_rep_hills = 0;

    // device-resident tail (tail_kernels.hip)
    bool use_gpu_tail = true;
    bool tail_on_device = false;          // results of the last construct live on the device
    bool host_stale = false;              // host mirrors (lists, graph, read state) need a download
    bool marks_on_device = false;         // transitive marks of the device graph not fetched yet
    uint32_t t_n0 = 0, t_n1 = 0, t_rounds = 0, t_n_kept = 0, t_n_nodes = 0, t_n_edges = 0, t_n_alive = 0;
    size_t t_med_tmp = 0;                 // bytes of d_med_tmp
    rala_hip::DevBuf<uint8_t> d_t_state, d_t_round, d_dirty, d_touched;
    rala_hip::DevBuf<uint32_t> d_n_pits0;
    rala_hip::DevBuf<uint16_t> d_cmed;
    rala_hip::DevBuf<uint8_t> d_med_tmp;
    rala_hip::DevBuf<uint32_t> d_cc_flags;
    rala_hip::DevBuf<uint32_t> d_kill[3], d_kill2[3], d_kill_count, d_death_sure;
    rala_hip::DevBuf<uint32_t> d_rank, d_alive_reads, d_t_tmp[2], d_kept_item, d_dovetail, d_epos, d_node_rank,
        d_node_read, d_e[3], d_t_death[2], d_t_work[2], d_t_fin, d_fp_map, d_fp_pack;
    rala_hip::DevBuf<uint8_t> d_t_mark;
    rala_hip::PinnedBuf<uint32_t> p_alive_reads, p_sens_rest;
    rala_hip::PinnedBuf<uint8_t> p_touched;
    rala_hip::PinnedBuf<uint16_t> p_cmed;

    // host tail
    std::vector<uint8_t> dirty, ever_dirty;       // reads whose valid region changed (this round / ever)
    std::vector<uint32_t> dirty_list;
    rala_hip::DevBuf<uint32_t> d_cc_edges, d_cc_label;
    rala_hip::DevBuf<uint32_t> d_tr[7];
    rala_hip::DevBuf<uint8_t> d_tr_marks;
    std::vector<rala_hip::HostOvl> overlaps, internals, scratch_ovl;
    std::vector<rala_hip::EdgePair> scratch_ep;
    std::vector<uint8_t> scratch_has, scratch_touched;
    std::vector<uint32_t> h_n_pits0;
    std::vector<uint32_t> scratch_u32a, scratch_u32b, scratch_u32c, alive_rank, alive_reads;
    rala_hip::PinnedBuf<uint32_t> p_cc_edges, p_cc_label;
    std::vector<uint32_t> node_read;
    std::vector<uint32_t> e_src, e_dst, e_len;
    std::vector<uint8_t> e_mark;

    rala_hip_timings tm = {};
};
