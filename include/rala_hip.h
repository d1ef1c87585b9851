/*
 * librala_hip — C ABI of the MI355X (gfx950) implementation of Rala's
 * data-parallel hot path: pile-o-gram construction / annotation from
 * PAF/MHAP overlaps, overlap filtering, assembly-graph edge construction and
 * transitive-edge reduction.
 *
 * The reference (rvaser/rala, C++11) has no FFI; these entry points are what
 * a binding of its hot path would call.  Each one names the reference
 * interface it replaces (paths relative to the reference root).  All calls
 * are blocking and are made from one host thread per context, like the
 * reference's public API (src/graph.hpp:37-117).  Return value: 0 on success,
 * a negative RALA_HIP_E* code otherwise; rala_hip_last_error() gives the text.
 * No CPU fallback exists: without a usable HIP device every call fails.
 *
 * Data model.  Reads are numbered 0..n_reads-1 in sequence-file order
 * (src/graph.cpp:255-259).  Overlaps are handed over as a structure of arrays
 * in file order; a_id/b_id are read numbers (a name that is not in the
 * sequence file is passed as RALA_HIP_NO_READ: Overlap::transmute returns
 * false for it, src/overlap.cpp:44-47).  `length` is PAF column 11, or the
 * larger span for MHAP (src/overlap.cpp:16,29); `strand` is 0 for '+' /
 * equal rc flags and 1 otherwise (src/overlap.cpp:19,30).
 */
#ifndef RALA_HIP_H_
#define RALA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RALA_HIP_NO_READ 0xFFFFFFFFu

enum {
    RALA_HIP_OK = 0,
    RALA_HIP_EDEVICE = -1,    /* HIP runtime error / no device */
    RALA_HIP_EINVAL = -2,     /* bad argument or call order */
    RALA_HIP_ECAPACITY = -3,  /* a fixed-capacity device list overflowed (raise via rala_hip_set_option) */
    RALA_HIP_EFILTERED = -4,  /* "filtered all sequences" (src/graph.cpp:418-421) */
    RALA_HIP_ENOMEM = -5,
    RALA_HIP_ENOTAFILE = -6,  /* the device tokeniser wants a regular file (a FIFO, a process substitution: take the host reader) */
    RALA_HIP_ETOOLARGE = -7   /* beyond the device tokeniser's 32-bit chunk / row counts (take the host reader) */
};

/* rala::OverlapType (src/overlap.hpp:27-33) */
enum { RALA_HIP_TYPE_X = 0, RALA_HIP_TYPE_A = 1, RALA_HIP_TYPE_B = 2, RALA_HIP_TYPE_AB = 3, RALA_HIP_TYPE_BA = 4 };

/* RALA_HIP_MEM_HOST_ASYNC (rala_hip_set_overlaps only): host memory - page-locked, if the copies are to run beside anything -
 * that stays valid until the next rala_hip_initialize has returned: the columns are then uploaded by that call, each in front
 * of the first kernel that reads it, on a stream of their own (ids -> the counting pass; b coordinates -> the first scatter;
 * a coordinates -> the query side; lengths, strands beside the pile kernels). */
enum { RALA_HIP_MEM_HOST = 0, RALA_HIP_MEM_DEVICE = 1, RALA_HIP_MEM_HOST_ASYNC = 2 };

typedef struct rala_hip_ctx rala_hip_ctx;

typedef struct rala_hip_overlaps {
    const uint32_t* a_id;
    const uint32_t* b_id;
    const uint32_t* a_begin;
    const uint32_t* a_end;
    const uint32_t* b_begin;
    const uint32_t* b_end;
    const uint32_t* length;
    const uint8_t* strand;
} rala_hip_overlaps;

/* Per-stage device time of the last rala_hip_construct / stage call, in
 * milliseconds (HIP events on the context's stream), and host time of the
 * sequential tail.  Duplicate removal runs on a second stream beside the bucketing and the
 * pile kernels: dedupe_ms is what it adds beyond them (normally 0). */
typedef struct rala_hip_timings {
    float dedupe_ms, bucket_ms, pile_ms, classify_ms, death_ms, finish_ms, tail_host_ms, tr_ms, total_ms;
    uint32_t pile_launches, death_rounds, pile_overflow_reads, pile_position_reads;
    /* reads whose slope-region / interval lists outgrew the LDS and ran with lists in global memory (initialize; the
     * sensitive pass adds its own); times an interval pool was grown and the stage repeated */
    uint32_t pile_unbounded_reads, pool_regrown;
    float repeats_ms;      /* the sensitive pass (Graph::preprocess, repeats: graph.cpp:882-1054), part of tail_host_ms */
} rala_hip_timings;

/* ---- context -------------------------------------------------------------- */
/* Replaces rala::createGraph's resource set-up (src/graph.cpp:184-238: parsers,
 * thread pool, logger) — here: device selection, one HIP stream, device arenas. */
int rala_hip_create(int device, rala_hip_ctx** out);
void rala_hip_destroy(rala_hip_ctx* ctx);
const char* rala_hip_last_error(const rala_hip_ctx* ctx);
/* options: "interval_pool_per_read_x1000" (default 1000 = one pit/hill slot per
 * read on average; a hint - a pool that turns out too small is grown to the counted need and the stage runs again), "max_lds_read_len" (position-space kernel: reads longer than this use
 * the HBM slab path), "use_run_kernel" (default 1; 0 sends every read through the
 * position-space kernel), "use_gpu_tail" (default 1; 0 runs the chimera stage of
 * Graph::preprocess on the host), "use_fixed_buckets" (default 1; 0 always buckets the bounds
 * through the exact count / scan / scatter path), "use_side_stream" (default 1; 0 runs duplicate
 * removal on the main stream before the bucketing and the pile chain's small kernels - event-dense
 * and longer reads - before its first one instead of beside it), "sensitive_in_device_memory" (default 0; 1 = the
 * sensitive overlaps handed to rala_hip_construct are device pointers), "host_threads",
 * "use_round_batches" (default 1: the containment fixed point of the second pass is finished on the device after two
 * rounds; 0 makes the host look at the killer list after every round), "use_partitioned_buckets" (default 1; 0 buckets the
 * target side through fixed slots), "debug_fp_lds_limit" (tests: containment fixed points with more killers than this
 * take the kernel for lists that do not fit the LDS), "debug_fp_give_up" (tests: 1 or 2 - the workgroups of that kernel do not
 * meet at their first barrier / at the later ones, and the last one to leave does the rounds alone), "use_fused_emit" (default 1; sharded runs: the senders scatter the
 * bounds once, by (owner, partition of the owner's reads), and the owners start at the second level of the partitioned
 * bucketing; 0: bounds grouped by owner only, bucketed by the owner from the start), "use_bound_records" (default 1; sharded
 * runs without the former: 0 ships two bound tuples per overlap side instead of one bound record),
 * "debug_part_shift" (tests / measurements: the partitioned bucketing's first-level partitions hold 1 << value reads,
 * 12 .. 14; 0 = by the rule - 4096 reads, more where that would make more than 256 partitions),
 * "pile_chunk_mb" (default 1024: the rows of all piles lie in physical chunks of this many MB mapped side by side into one range -
 * hipMemCreate / hipMemMap - which the first pile kernel's stores like better than where one hipMalloc puts them; 0 = one hipMalloc),
 * "pile_rows" (default 1: the coverage rows of all piles are resident, 2 bytes per base; 0, read by the next rala_hip_initialize:
 * no row is allocated or stored - a row is a pure function of the read's bound events, which stay on the device anyway, and is
 * rebuilt from them whenever a getter or the sensitive pass asks; every call answers what it answers with 1, except that
 * rala_hip_get_pile_row_digests' `outside` is 0, and one rala_hip_initialize takes one sensitive construct - see
 * rala_hip_get_pile_rows_info), "pile_rows_scratch_mb" (default 256: with pile_rows = 0, the device memory a batch of rebuilt rows
 * may take; it grows to the longest single row),
 * "debug_chunk_fail" (tests: the mapping of those chunks fails at chunk k, and the rows come from one hipMalloc; -1, the default: never),
 * "debug_count_window" (tests: the partitioned bucketing counts this many groups of 128 reads per pass over the ids;
 * 0 = what a workgroup's LDS holds, 38 400 - one pass up to 4.9 M reads),
 * "debug_ev_events" (tests / measurements: 1 = the partitioned bucketing's row offsets count bound events where 4 n fits 32 bits, as
 * before round 6; 0, the default: bound pairs - up to 2^31 overlaps per context),
 * "debug_dedupe_list_cap" (tests: the list of the runs duplicate removal's counting pass marks holds this many marks, 0 = the
 * default 2^20; a list that does not hold them all is given up and the pass over all overlaps does the work),
 * "gzip_on_device" (default 0; 1: rala_hip_set_overlaps_from_paf / _mhap inflate a single-member gzip file on the device, see there),
 * "gzip_in_pieces" (default 0; with "gzip_on_device" 1: the ranks of a sharded run take such a file together, see rala_hip_mg_set_overlaps_from_mhap),
 * "gzip_members" (default 0; with "gzip_on_device" 1: a gzip file of SEVERAL members that is not BGZF - cat a.gz b.gz, pigz -i,
 * a .gz file that was appended to - is walked member by member on the device instead of refused, see rala_hip_gzip_chain_members),
 * "gzip_chunk_bytes" (default 65536: the compressed bytes one wave of that inflater starts in; at least 1024),
 * "debug_gzip_false_sync" (tests: every n-th of those chunks is given a bogus block start at its first bit; 0, the default: none),
 * "debug_sequence_window" (tests: rala_hip_index_sequences takes the read file's text through windows of this many bytes; 0, the
 * default: a quarter of the free device memory, 2 GiB at most),
 * "layout_fused_max" (default 1024; rala_hip_layout_batch: a component of at most this many points is laid out by one workgroup
 * in one launch, a larger one step by step with all other larger ones; 0: none is fused; a value above 1024 - what a workgroup's
 * threads and LDS hold - or below 0 is RALA_HIP_EINVAL),
 * "debug_pile_stop_after" (diagnostics: leave the run-space pile kernel after phase k, 99 = all;
 * 100 * m + k: the same without the row stores (m = 1), tools/phase_probe.py) */
int rala_hip_set_option(rala_hip_ctx* ctx, const char* key, int64_t value);
/* the context's hipStream_t, for callers that enqueue their own copies/collectives */
void* rala_hip_stream(rala_hip_ctx* ctx);

/* ---- inputs ------------------------------------------------------------------ */
/* Replaces the createPile loop of Graph::initialize (src/graph.cpp:249-264). */
int rala_hip_set_reads(rala_hip_ctx* ctx, const uint32_t* read_len, uint64_t n_reads);
/* Replaces the overlap stream of both parser passes (src/graph.cpp:328-382, :443-518):
 * parsed once, kept as binary SoA in HBM.  mem = RALA_HIP_MEM_HOST copies from host
 * memory; RALA_HIP_MEM_DEVICE adopts device pointers, which must stay valid; RALA_HIP_MEM_HOST_ASYNC
 * leaves the copies to rala_hip_initialize (above). */
int rala_hip_set_overlaps(rala_hip_ctx* ctx, const rala_hip_overlaps* ovl, uint64_t n, int mem);

/* The same from PAF TEXT, tokenised on the device (uncompressed files).  Replaces bioparser's PAF parser and the two
 * hash look-ups of Overlap::transmute (src/graph.cpp:328-352, src/overlap.cpp:36-82): `threads` reader threads ship the
 * file to the device in blocks (pinned staging, copies overlapped with the reads), two kernels count the lines and parse
 * them - one thread per line: names cut at the first blank and looked up in the name table, numbers as their leading
 * digits, column 11 as the overlap's length, the strand, Overlap::transmute's length check (check_lengths: the first
 * record in file order whose length differs from its sequence's is returned in *length_error_read, -1 = none; the
 * caller prints the reference's message).  The columns stay on the device and are the context's overlaps afterwards.
 * *irregular != 0: the file is not a plain list of 12-column records (a line with fewer columns, a name of more than a
 * kilobyte ...) - nothing was set, take the host reader (rala_amd/host/io.cpp), which knows what to do with such files.
 * The name table: rala::io::NameTable as built on the host (rala_amd/csrc/name_table.h: 32-byte buckets {hash32, id + 1,
 * length, arena offset, first 16 bytes}, n_buckets a power of two, the names' bytes in `arena`).
 * A BGZF file (what bgzip writes: gzip members of at most 64 KB with a "BC" extra field) is taken as well: the compressed
 * bytes go to the device, a kernel inflates the members into the text the plain file would have given, and the same
 * kernels tokenise it (ship_ms then counts the compressed bytes; rala_hip_get_inflate_timings: the inflater).  The members
 * accepted are those the host reader's BgzfSource accepts (rala_amd/host/io.cpp); anything else - a plain single-member
 * gzip stream (known from its first 18 bytes, before anything is shipped), a cut file, a bad CRC32 or ISIZE, bytes behind
 * the last member that are no member - gives *irregular & 8 and sets nothing.
 * With the option "gzip_on_device" set, any other gzip file of ONE member (what gzip, pigz, Python's gzip and `minimap2 | gzip`
 * write; with bioparser's gzread loop the reference's only compressed input, src/graph.cpp:190-224, 328-352) is inflated on
 * the device as well, by speculative decoding: the deflate bytes are cut into chunks of "gzip_chunk_bytes", every chunk finds
 * the first bit in it that can start a block and is decoded from there without knowing the 32 KB in front of it, into 16-bit
 * symbols (a byte, or "byte k of the window in front of this chunk"); the chain of chunks that ended at each other's starts
 * from chunk 0 is the stream, the rest is dropped; windows and symbols are resolved in text order, and the result is
 * proved: CRC32, ISIZE mod 2^32, the final block ending exactly at the 8 trailer bytes.  Anything else - a header RFC 1952
 * does not allow, an invalid block, a cut stream, a second member (unless the option "gzip_members" is set, see
 * rala_hip_gzip_chain_members) or other bytes behind the trailer - gives *irregular & 8 and sets nothing.  The compressed bytes, two bytes per byte of text and the text must fit in device memory together
 * (RALA_HIP_ENOMEM otherwise; the caller takes the host reader).  rala_hip_get_gzip_timings: the passes. */
typedef struct rala_hip_ingest_timings {
    float ship_ms;          /* file -> device memory (reads and copies overlapped) */
    float tokenize_ms;      /* count + scan + parse on the device */
    uint64_t bytes, lines;
} rala_hip_ingest_timings;
int rala_hip_set_name_table(rala_hip_ctx* ctx, const void* buckets, uint64_t n_buckets, const char* arena, uint64_t arena_bytes);
int rala_hip_set_overlaps_from_paf(rala_hip_ctx* ctx, const char* path, int check_lengths, uint32_t threads,
                                   int64_t* length_error_read, int* irregular);
/* The same for an uncompressed MHAP file (round 6): bioparser's MhapParser and the MHAP constructor of Overlap
 * (src/overlap.cpp:12-20) - twelve blank-separated columns "a_id b_id error minmers a_rc a_begin a_end a_length b_rc b_begin
 * b_end b_length", all numbers: id = the column minus one (ids are counted from 1; one that names no read does not
 * resolve), length = the longer of the two spans, strand = a_rc != b_rc, the length check of Overlap::transmute on columns
 * 8 and 12.  No name table is needed.  *irregular as above (fewer than twelve columns, ...). */
int rala_hip_set_overlaps_from_mhap(rala_hip_ctx* ctx, const char* path, int check_lengths, uint32_t threads,
                                    int64_t* length_error_read, int* irregular);
int rala_hip_get_ingest_timings(rala_hip_ctx* ctx, rala_hip_ingest_timings* out);
/* The inflater of the last rala_hip_set_overlaps_from_paf / _mhap call (zeros when the file was not BGZF). */
typedef struct rala_hip_inflate_timings {
    float inflate_ms;           /* the members inflated on the device (all windows) */
    uint64_t compressed_bytes;  /* the file's bytes shipped to the device */
    uint64_t members;           /* gzip members with text */
} rala_hip_inflate_timings;
int rala_hip_get_inflate_timings(rala_hip_ctx* ctx, rala_hip_inflate_timings* out);
/* The speculative inflater of the last rala_hip_set_overlaps_from_paf / _mhap call (zeros when it did not run), or of the last
 * rala_hip_index_sequences of a single-member gzip file.  rala_hip_slice_sequences of such a file overwrites them with its own
 * walk: it takes the index's chain over, so find_ms, chunks, chunks_with_candidate and chunks_refuted are 0 then, and decode_ms
 * is the writing pass alone. */
typedef struct rala_hip_gzip_timings {
    float find_ms;                  /* block starts searched in every chunk */
    float decode_ms;                /* the counting pass and the writing pass */
    float resolve_ms;               /* windows, symbols -> text, CRC32 */
    uint64_t compressed_bytes;      /* the file's bytes shipped to the device */
    uint64_t text_bytes;
    uint64_t chunks;                /* chunks of gzip_chunk_bytes, the first one included */
    uint64_t chunks_with_candidate; /* of the others: a candidate block start was found */
    uint64_t chunks_confirmed;      /* of those: on the chain from chunk 0 (the stream was decoded by this many waves + 1) */
    uint64_t chunks_refuted;        /* of those: passed by a wave of the chain that did not land on them */
    uint64_t max_wave_text_bytes;   /* the most text one wave of the chain produced */
} rala_hip_gzip_timings;
int rala_hip_get_gzip_timings(rala_hip_ctx* ctx, rala_hip_gzip_timings* out);
/* The header of a gzip member (RFC 1952) in the first n bytes of a file (no context, no device), as the device ingest reads
 * it: ID1 ID2, CM = 8, FLG with FEXTRA / FNAME / FCOMMENT / FHCRC and its reserved bits clear.  *valid = 1: the deflate
 * bytes begin at *deflate_off; 0: not such a header, or it does not end within the n bytes. */
int rala_hip_gzip_head(const uint8_t* bytes, uint64_t n, uint64_t* deflate_off, int* valid);
/* The chain of true chunks of a single-member gzip stream (no context, no device), as the device ingest builds it from what
 * the device found and counted in each of n_chunks chunks - starts[c]: the bit chunk c's first candidate block begins at
 * (~0: none); status[c]: 0 decoding from there ended at the start of chunk next[c], 1 the final block ended at bit end_bit[c],
 * 2 invalid, 3 no start; text[c]: the bytes it gives; refuted[c]: later starts it passed - followed from chunk 0.  end: the
 * trailer's first byte; isize: the trailer's ISIZE.  *valid = 0, refused: a chunk on the chain with status > 1, a next that
 * does not lead forward to a chunk there is, a final block that does not end in the byte in front of `end`, a text whose size
 * is not isize modulo 2^32.  *n_jobs: the chain's chunks; when cap >= *n_jobs, each one's first bit, the bit it stops at (~0:
 * the final block's end), its text offset and text size are written to the arrays given (any may be null).  stats (may be
 * null): chunks, chunks_with_candidate, chunks_confirmed, chunks_refuted, max_wave_text_bytes and text_bytes of the walk. */
int rala_hip_gzip_chain(const uint64_t* starts, const uint64_t* end_bit, const uint64_t* text, const uint32_t* next,
                        const uint32_t* status, const uint32_t* refuted, uint64_t n_chunks, uint64_t end, uint32_t isize, uint64_t cap,
                        uint64_t* n_jobs, uint64_t* start_bit, uint64_t* stop_bit, uint64_t* text_off, uint64_t* text_n,
                        rala_hip_gzip_timings* stats, int* valid);
/* ---- gzip files of several members (option "gzip_members" beside "gzip_on_device") -----------------------------------------
 * The reference reads `cat a.fastq.gz b.fastq.gz` and `cat part*.paf.gz` transparently: bioparser's gzread walks from member to
 * member (src/graph.cpp:190-224, 249-264, 328-352).  With both options set, rala_hip_set_overlaps_from_paf / _mhap,
 * rala_hip_index_sequences and rala_hip_slice_sequences do the same on the device: a kernel finds every byte offset at which a
 * member header begins (rala_hip_gzip_head's parse; a magic inside deflate bytes is found too and never reached), the counting
 * pass also decodes from every such header's first block as from a stream's first chunk, and the host walks the chain: where a
 * final block ends, the next 8 bytes are the member's trailer - its ISIZE must be the member's text size modulo 2^32 - and
 * either the file ends behind them or a found header begins there.  Every member is proven separately: a back reference that
 * reaches in front of its member's first byte is refused (zlib refuses it), and every member's CRC32 is compared with its own
 * trailer.  Anything else - bytes between or behind members that are no header, a cut member, a wrong inner CRC32 or ISIZE -
 * gives *irregular & 8 and sets nothing.  With "gzip_members" 0 a second member is refused as before.
 *
 * The chain of such a file (no context, no device), in the style of rala_hip_gzip_chain: besides the chunks' arrays, n_cands
 * member candidates in ascending order - cand_header_off[k]: the header's first byte, cand_deflate_bit[k]: the bit its deflate
 * bytes begin at, cand_prev_crc / cand_prev_isize[k]: the 8 bytes in front of the header, cand_end_bit / cand_text / cand_next /
 * cand_status[k]: what decoding from cand_deflate_bit[k] as a first chunk gave.  file_n: the file's size; last_crc, last_isize:
 * its last 8 bytes.  *valid = 0, refused: what rala_hip_gzip_chain refuses, a trailer behind which neither the file ends nor
 * a candidate begins, a member whose text size is not its ISIZE, a member cut by the file's end, an end_bit or a next that
 * does not lead forward.  Jobs as rala_hip_gzip_chain gives them, and first[j] = 1 on every member's first job; members
 * (when member_cap >= *n_members): each one's text offset, text size and the CRC32 its trailer names, empty members included. */
int rala_hip_gzip_chain_members(const uint64_t* starts, const uint64_t* end_bit, const uint64_t* text, const uint32_t* next,
                                const uint32_t* status, const uint32_t* refuted, uint64_t n_chunks, const uint64_t* cand_header_off,
                                const uint64_t* cand_deflate_bit, const uint32_t* cand_prev_crc, const uint32_t* cand_prev_isize,
                                const uint64_t* cand_end_bit, const uint64_t* cand_text, const uint32_t* cand_next,
                                const uint32_t* cand_status, uint64_t n_cands, uint64_t file_n, uint32_t last_crc, uint32_t last_isize,
                                uint64_t cap, uint64_t* n_jobs, uint64_t* start_bit, uint64_t* stop_bit, uint64_t* text_off,
                                uint64_t* text_n, uint32_t* first, uint64_t member_cap, uint64_t* n_members, uint64_t* member_text_off,
                                uint64_t* member_text_n, uint32_t* member_crc32, rala_hip_gzip_timings* stats, int* valid);
/* The member find alone (tests): the n bytes are shipped to the device and every offset at which rala_hip_gzip_head takes the
 * bytes from there on (at most 2^20 of them) is returned in ascending order - *n_found of them; when cap >= *n_found, each
 * header's offset and where its deflate bytes begin. */
int rala_hip_gzip_find_members(rala_hip_ctx* ctx, const uint8_t* bytes, uint64_t n, uint64_t cap, uint64_t* n_found, uint64_t* header_off,
                               uint64_t* deflate_off);
/* The members of the gzip file the last rala_hip_set_overlaps_from_paf / _mhap or rala_hip_index_sequences inflated on the
 * device (none: it inflated none, or refused): *n of them; when cap >= *n, each one's text offset, text size and CRC32. */
int rala_hip_get_gzip_members(rala_hip_ctx* ctx, uint64_t* n, uint64_t cap, uint64_t* text_off, uint64_t* text_n, uint32_t* crc32);
/* The member index of a BGZF file held in memory (no context, no device): the chain of gzip members from byte 0, as the
 * device ingest builds it - the bytes scanned for member headers in blocks of block_bytes (0: the ingest's 32 MB), then
 * walked from offset 0.  *valid = 0: not a BGZF file the host reader would take (first 18 bytes not a BGZF header, a cut
 * member, bytes behind the last member that are no member, ISIZE > 65536).  *n_members: the members (empty ones included);
 * when cap >= *n_members, each one's file offset, compressed size (BSIZE + 1), text size (ISIZE) and text offset (the
 * exclusive scan of the text sizes) are written to the arrays given (any may be null). */
int rala_hip_bgzf_index(const uint8_t* bytes, uint64_t n, uint64_t block_bytes, uint64_t cap, uint64_t* n_members, uint64_t* file_off,
                        uint32_t* comp_bytes, uint32_t* text_bytes, uint64_t* text_off, int* valid);
/* A BGZF file in PIECES by compressed byte range (no context, no device; what a rank of a sharded run does with its share of
 * the file, rala_hip_mg_set_overlaps_from_paf with the option "bgzf_in_pieces"): the piece [lo, hi) of the n bytes holds the
 * members whose header BEGINS in it - found by the same scan over blocks of block_bytes (0: 32 MB) that start at lo, walked as
 * a chain from the first candidate in the range until the chain reaches an offset >= hi, where a candidate or the file's end
 * must stand; a member's ISIZE is read from the 4 bytes in front of the next header.  Nothing in front of lo is looked at
 * (but the 8 bytes in front of a block).  *begin: the offset of the piece's first member; *end: the offset the chain
 * reached; *empty: no header begins in the range.  *valid = 0: the chain broke (what rala_hip_bgzf_index refuses), or lo = 0
 * and the first 18 bytes are no BGZF header.  A piece that is valid says nothing about the file: the caller joins the pieces
 * with rala_hip_bgzf_pieces_chain.  When cap >= *n_members, each member's file offset, compressed size and text size. */
int rala_hip_bgzf_index_range(const uint8_t* bytes, uint64_t n, uint64_t lo, uint64_t hi, uint64_t block_bytes, uint64_t cap,
                              uint64_t* n_members, uint64_t* file_off, uint32_t* comp_bytes, uint32_t* text_bytes, uint64_t* begin,
                              uint64_t* end, int* empty, int* valid);
/* 1: the n_pieces pieces (in file order) are one chain of members from offset 0 to file_bytes - piece 0 is not empty and begins
 * at 0, every piece that is not empty begins where the one in front of it ended, the last of them ends at file_bytes.  0: a
 * gap, a false candidate that started a piece's chain, a cut file - the host reader decides (src/graph.cpp:190-224). */
int rala_hip_bgzf_pieces_chain(const uint64_t* begin, const uint64_t* end, const int* empty, uint32_t n_pieces, uint64_t file_bytes);
/* ---- the read file: names, lengths and offsets of every sequence, indexed on the device ---------------------------------
 * Replaces the first sequence pass of Graph::initialize (src/graph.cpp:249-264: bioparser's FASTA / FASTQ parser, a heap
 * Sequence per read of which the name and the length are kept) and lets the second one (src/graph.cpp:527-551) cut the
 * bases of the reads the graph keeps out of the file instead of parsing it again.  format 0: FASTA - a record starts with
 * '>' at byte 0 of the text or directly behind a newline, its name ends at the first blank, tab or line end, its bases are
 * the lines up to the next record, newlines (and a carriage return in front of one) taken out; bytes in front of the first
 * '>' are ignored.  format 1: FASTQ of four lines per record - a header that is not empty, bases, a line that starts with
 * '+', qualities as long as the bases.  The text goes through device memory in windows (`threads` reader threads, pinned
 * staging, as for the overlaps; option "debug_sequence_window": the window's bytes, for tests); a BGZF file is inflated on
 * the device, offsets are then offsets into its text.  What the host readers (rala_amd/host/io.cpp: read_fasta, read_fastq)
 * give for such a file is what this gives.  *irregular != 0: nothing was set, the context's reads are what they were - take
 * the host reader: 1 FASTQ of another shape (multi-line records, blank lines, a cut record, a quality line of another
 * length), 2 a name of more than 1024 bytes, 4 a header line of more than 4096 bytes, 8 a gzip file that is not BGZF (known
 * from its first 18 bytes) or a BGZF file the inflater refuses.  A FIFO: RALA_HIP_ENOTAFILE; a read of 2^32 bases or more:
 * RALA_HIP_ETOOLARGE.  After a successful call the lengths are the context's reads, as rala_hip_set_reads leaves them. */
int rala_hip_index_sequences(rala_hip_ctx* ctx, const char* path, int format, uint32_t threads, uint64_t* n_records,
                             uint64_t* name_bytes, int* irregular);
/* The index of the last successful rala_hip_index_sequences (bioparser's FASTA / FASTQ parsers, per record what they put into a
 * Sequence: src/sequence.cpp:11-23), n_records entries each, any pointer may be NULL: the name = name_len bytes at names +
 * name_off (names: name_bytes bytes, the names in record order); the bases = the length bytes that remain of the text
 * [data_off, data_off + data_span) when every newline and every carriage return in front of one is taken out. */
int rala_hip_get_sequence_index(rala_hip_ctx* ctx, uint64_t* name_off, uint32_t* name_len, uint64_t* data_off,
                                uint64_t* data_span, uint32_t* length, char* names);
/* ship_ms: the file (BGZF: its compressed bytes) to the device; tokenize_ms: the kernels (BGZF: the inflater among them);
 * bytes: the text's; lines: the records (the "loaded sequences" stage of src/graph.cpp:246-266) */
int rala_hip_get_sequence_timings(rala_hip_ctx* ctx, rala_hip_ingest_timings* out);
/* The name table built on the device from the index of the last successful rala_hip_index_sequences, and installed exactly where
 * rala_hip_set_name_table would have put the host's (replaces reference src/graph.cpp:249-264: one string per read into an
 * unordered_map - here the host's string-plus-map loop, NameTable::build and the upload of its table): the same buckets, hash
 * (rala_amd/csrc/name_table.h) and capacity - the smallest power of two not below 2 n + 2, at least 16 -, a later record of a name
 * takes it as in NameTable::build; the arena is a device-to-device COPY of the index's names (a later rala_hip_index_sequences does
 * not touch the table), a bucket's `off` its read's name_off.  Every look-up answers as in the host's table; which name sits
 * in which slot of a probe path may differ from it, and from run to run.  *n_buckets: the capacity; *n_distinct: the taken buckets.
 * RALA_HIP_EINVAL: no index; RALA_HIP_ETOOLARGE: 2^32 bytes of names or more (`off` has 32 bits), or 2^32 - 1 records or more
 * (id1 = id + 1); RALA_HIP_EDEVICE where a probe path did not end within n_buckets steps (every probe loop is bounded).  After any
 * refusal the table installed before is still there, untouched: take the host's build. */
int rala_hip_build_name_table(rala_hip_ctx* ctx, uint64_t* n_buckets, uint64_t* n_distinct);
/* The installed table read back, whoever installed it (reference src/graph.cpp:249-264: the map it stands for): n_buckets 32-byte
 * buckets and arena_bytes bytes of names.  buckets and arena may be NULL: the sizes only.  RALA_HIP_EINVAL: no table installed. */
int rala_hip_get_name_table(rala_hip_ctx* ctx, void* buckets, char* arena, uint64_t* n_buckets, uint64_t* arena_bytes);
/* src's installed table copied into dst, device to device (the contexts of a sharded run's ranks, the shares of -s: the map of
 * reference src/graph.cpp:249-264 once per context) - through pinned host memory where the two devices have no peer access. */
int rala_hip_copy_name_table(rala_hip_ctx* dst, rala_hip_ctx* src);
/* The table's hash of the n bytes at p, on the host: no context, no device (name_table.h's name_hash_with, the one definition; the
 * key of the map of reference src/graph.cpp:249-264). */
uint64_t rala_hip_name_hash(const char* p, uint64_t n);
/* The last rala_hip_build_name_table of the context that succeeded (zeros before the first; reference src/graph.cpp:249-264 is what
 * it replaces). */
typedef struct rala_hip_name_table_info {
    uint64_t names;             /* records of the index */
    uint64_t distinct;          /* taken buckets */
    uint64_t n_buckets;
    uint32_t longest_probe;     /* slots the longest insert looked at */
    float device_ms;            /* between two HIP events around the clear, the two kernels and the arena's copy */
} rala_hip_name_table_info;
int rala_hip_get_name_table_info(rala_hip_ctx* ctx, rala_hip_name_table_info* out);
/* With the option "gzip_on_device" set, rala_hip_index_sequences takes a gzip file of ONE member that is not BGZF as well (what
 * gzip, pigz and basecallers write).  The compressed bytes stay in device memory while the file is indexed - the only buffer
 * whose size depends on the file's; block starts are found and the chain from chunk 0 is followed as for the overlaps (see
 * rala_hip_set_overlaps_from_paf), and the text is then written and resolved WINDOW by window: a window is a run of true
 * chunks whose text fits it (a quarter of the free memory over three bytes per text byte; option "debug_sequence_window";
 * never less than the largest chunk's text - RALA_HIP_ENOMEM where that does not fit), the last 32 768 bytes of a window are
 * carried in front of the next one's symbols, the windows' CRC registers are chained.  CRC32, ISIZE and the final block ending
 * at the trailer prove the text; anything else - several members included, unless the option "gzip_members" is set: then every
 * member is proven so, any number of member boundaries in a window - is *irregular = 8.  The index equals that of the
 * uncompressed file.  rala_hip_get_gzip_timings then speaks of this call.
 *
 * The second pass: the bases of the reads `wanted` (ascending record numbers of the current index, n_wanted of them) are cut
 * out of the file on the device and written packed to `bases` (host memory): read wanted[k]'s at bases + base_off[k], where
 * base_off (n_wanted + 1 entries) is the exclusive scan of the wanted reads' lengths.  The call walks the text in the windows
 * of the index pass - a plain file's bytes, a BGZF file's members, a gzip member's chunks again (the chain is the context's;
 * the compressed bytes are shipped once more) - and gathers every window's share with one kernel; the output leaves the device
 * window by window.  *irregular != 0: refused, `bases` holds nothing of use, take the host reader - 64 there is no index or the
 * file's size is not what the index saw, 8 the inflater refused or the gzip text's CRC32 / ISIZE are no longer the index's,
 * 32 the text does not fit the index in another way. */
int rala_hip_slice_sequences(rala_hip_ctx* ctx, const char* path, const uint64_t* wanted, uint64_t n_wanted, const uint64_t* base_off,
                             uint8_t* bases, uint32_t threads, int* irregular);
/* The last rala_hip_slice_sequences. */
typedef struct rala_hip_sequence_slice_info {
    uint64_t windows;               /* windows of text walked */
    uint64_t max_window_text_bytes; /* the most text one window held (the look-ahead behind it included) */
    uint64_t bases;                 /* bases written */
    float ship_ms;                  /* the file's bytes (compressed ones where it is compressed) to the device */
    float kernel_ms;                /* everything on the device: inflate, count, gather, the output's way back */
    float gather_ms;                /* of those: the gather kernel */
    float copy_ms;                  /* of those: the packed bases device -> host */
} rala_hip_sequence_slice_info;
int rala_hip_get_sequence_slice_info(rala_hip_ctx* ctx, rala_hip_sequence_slice_info* out);
/* ---- node bases as spans: a table of bases on the device, and the bytes that lists of spans of it spell ----------------
 * The nodes of the assembly graph need no base between Graph::construct and the output (src/graph.cpp:133-170 concatenates
 * strings for every unitig, :2042-2116 prints them): a node is a list of spans of reads, and its bytes are written once.
 *
 * The table belongs to the context and to nothing else in it: rala_hip_set_reads, rala_hip_initialize and rala_hip_construct
 * neither need nor drop it, rala_hip_destroy frees it; one table per context.  Source s is bases[base_off[s] .. base_off[s + 1])
 * - base_off always HOST memory (n_sources + 1 entries, kept by the context to check spans against), `bases` host
 * (RALA_HIP_MEM_HOST) or device memory (RALA_HIP_MEM_DEVICE); either way the bytes are COPIED into the context.  The call
 * replaces an earlier table; n_sources = 0 releases it.  RALA_HIP_EINVAL: offsets that decrease or do not begin at 0 - the
 * table that was there stays; RALA_HIP_ENOMEM leaves no table.
 * With the option "keep_bases" set, a successful rala_hip_slice_sequences leaves the packed bases it gathered on the device as
 * this table - source k the whole read wanted[k], the offsets its base_off; its `bases` may then be NULL and nothing is copied
 * to the host.  The windows' gather then writes into one buffer of the full size: RALA_HIP_ENOMEM for it is returned with
 * nothing set (repeat the call without the option); *irregular != 0 leaves no table. */
int rala_hip_set_bases(rala_hip_ctx* ctx, const uint8_t* bases, const uint64_t* base_off, uint64_t n_sources, int mem);
/* Bytes [first, first + len) of source `source`: out[j] = B[first + j], or (rc = 1) out[j] = comp(B[first + len - 1 - j]) with
 * comp A <-> T, C <-> G in upper case and every other byte unchanged (Sequence::create_reverse_complement, src/sequence.cpp).
 * A span of length 0 spells nothing. */
typedef struct rala_hip_span {
    uint32_t source, first, len, rc;
} rala_hip_span;
/* out (host memory, out_bytes bytes) receives what the spans spell, one after the other; where one record ends and the next
 * begins is the caller's business.  Checked on the host before anything is enqueued - a refused call touches nothing
 * (RALA_HIP_EINVAL): there is a table, source < n_sources, first + len within the source (64-bit arithmetic), rc 0 or 1, the
 * lengths sum to out_bytes; n_spans >= 2^32: RALA_HIP_ETOOLARGE.  n_spans = 0 or out_bytes = 0 enqueues nothing.  The output
 * leaves the device in windows (option "spell_window_mb", 256; "debug_spell_window": bytes, rounded down to whole 16 KB tiles,
 * one at least): one launch and one copy per window. */
int rala_hip_spell(rala_hip_ctx* ctx, const rala_hip_span* spans, uint64_t n_spans, uint8_t* out, uint64_t out_bytes);
/* The table, and the last rala_hip_spell. */
typedef struct rala_hip_spell_info {
    uint64_t sources, source_bytes; /* the table (0, 0: none) */
    uint64_t spans, bytes;          /* the last call: spans taken, bytes spelled */
    uint64_t windows, launches;
    float upload_ms;                /* the spans and their output offsets to the device */
    float kernel_ms;                /* the windows' kernels */
    float copy_ms;                  /* the windows' bytes device -> host */
    uint32_t from_slice;            /* 1: the table is what rala_hip_slice_sequences gathered (option "keep_bases") */
} rala_hip_spell_info;
int rala_hip_get_spell_info(rala_hip_ctx* ctx, rala_hip_spell_info* out);
/* The CRC32 of n pieces laid end to end (no context, no device), from every piece's CRC REGISTER - started from zero, no final
 * inversion: zlib's crc32(piece) ^ crc32(as many zero bytes) - and its length: how the windowed inflater chains its windows. */
uint32_t rala_hip_crc32_chain(const uint32_t* reg, const uint64_t* len, uint64_t n);
/* The sensitive overlaps (rala -s; Graph::preprocess, src/graph.cpp:901-939) of an uncompressed PAF file the same way, without
 * the length check (Overlap::transmute_ has none, src/overlap.cpp:84-114): the lines that start in bytes [lo, hi) of the file
 * (hi = ~0: to its end; a rank of a sharded run takes a share - any split of the sensitive set will do).  *out receives DEVICE
 * pointers that stay the context's (valid until the next call): hand them to rala_hip_construct / rala_hip_mg_run with the
 * option "sensitive_in_device_memory" set.  *irregular != 0: nothing was set, take the host reader. */
int rala_hip_tokenise_sensitive_paf(rala_hip_ctx* ctx, const char* path, uint64_t lo, uint64_t hi, uint32_t threads,
                                    rala_hip_overlaps* out, uint64_t* n, int* irregular);
/* The same for part `part` of `parts` of a sensitive file of any kind (src/graph.cpp:901-939), format 0: PAF, 1: MHAP (no name
 * table needed), no length check in either.  The parts are byte ranges of the FILE, [F / P k + min(k, F % P), ...).  Plain text:
 * the lines that start in the part's bytes.  BGZF: the part's piece (rala_hip_bgzf_index_range), inflated on the device; a
 * line belongs to the piece that holds the byte in front of its first byte.  Any other gzip file: parts = 1 and the option
 * "gzip_on_device" (and "gzip_members"), otherwise *irregular = 8.  piece[0 .. 2] = begin, end, empty of the part (plain text:
 * its byte range): there is no collective here, the caller of several parts checks rala_hip_bgzf_pieces_chain behind them
 * and takes the host reader where it fails.  The compressed bytes and the text are released before the call returns - the
 * context holds piles by then; RALA_HIP_ENOMEM is an answer to fall back on. */
int rala_hip_tokenise_sensitive(rala_hip_ctx* ctx, const char* path, int format, uint32_t part, uint32_t parts, uint32_t threads,
                                rala_hip_overlaps* out, uint64_t* n, uint64_t piece[3], int* irregular);
/* the context's overlap columns, wherever they came from, into host buffers (*n entries each; cols / strand may be NULL to
 * ask for the count alone): a_id, b_id, a_begin, a_end, b_begin, b_end, length */
int rala_hip_get_overlap_columns(rala_hip_ctx* ctx, uint64_t* n, uint32_t* const cols[7], uint8_t* strand);

/* ---- stages ---------------------------------------------------------------------- */
/* Graph::initialize (src/graph.cpp:244-425): duplicate removal (:273-307), bound
 * emission (:311-326), Pile::add_layers for every read (:367-377), then per read
 * find_valid_region / find_median / find_chimeric_hills / find_chimeric_pits (:387-407).
 * Returns RALA_HIP_EFILTERED if no read survives. */
int rala_hip_initialize(rala_hip_ctx* ctx);
/* Graph::construct after initialize (src/graph.cpp:437-640): second overlap pass with
 * the in-order containment removal (:443-518), Graph::preprocess for chimeras
 * (:699-880), optionally Graph::preprocess for repeats with a sensitive overlap set
 * (:882-1054; pass sens = NULL / n_sens = 0 for none), node and edge construction
 * (:553-632).  Sensitive overlaps: a = query in untrimmed coordinates, b = target in
 * TRIMMED coordinates (misc/raven.sh), host memory. */
int rala_hip_construct(rala_hip_ctx* ctx, const rala_hip_overlaps* sens, uint64_t n_sens);
/* Pile::find_repetitive_hills(dataset_median) of ONE read on its current coverage (src/pile.cpp:500-566)
 * with the Pile's members begin_, end_, median_, p10_ as given: slopes at 1.42, the 0.84 / 0.9 / 0.336
 * rules; the read's repeat hills (flags cleared) are then what rala_hip_get_intervals(kind 2)
 * reports for it.  The sensitive pass of rala_hip_construct does this for all reads; this entry
 * point serves a stand-alone rala::Pile. */
int rala_hip_find_repetitive_hills(rala_hip_ctx* ctx, uint64_t read, uint32_t begin, uint32_t end, uint16_t median,
                                   uint16_t p10, uint16_t dataset_median);
/* Graph::remove_transitive_edges on the graph built by rala_hip_construct
 * (src/graph.cpp:1281-1335).  *n_pairs = its return value. */
int rala_hip_remove_transitive_edges(rala_hip_ctx* ctx, uint32_t* n_pairs);
/* The same on a caller-supplied graph (host arrays): edge e and e^1 are
 * reverse-complement twins (Edge::pair_), out-lists are in edge-id order.
 * marks[e] = 1 for every edge the reference would mark. */
int rala_hip_tr_mark(rala_hip_ctx* ctx, uint32_t n_nodes, uint32_t n_edges, const uint32_t* src,
                     const uint32_t* dst, const uint32_t* len, uint8_t* marks, uint32_t* n_pairs);

/* ---- multi-GPU building blocks (one process per GPU; the collective itself is the caller's,
 * e.g. RCCL through torch.distributed).  Reads are partitioned over ranks; rank k holds a
 * slice of the overlap file cut on a_id-run boundaries. ---------------------------------- */
/* remove_duplicate_overlaps only (src/graph.cpp:273-307) on this context's overlaps */
int rala_hip_dedupe(rala_hip_ctx* ctx);
/* A bound tuple is 8 bytes: the read in the low 32 bits, the bound ((position << 1) | is_end,
 * src/graph.cpp:317-324) in the high 32 bits - one element of the ONE all-to-all that ships every
 * bound to the owner of its read.
 * store_overlap_bounds (src/graph.cpp:311-326) as tuples: for overlap i the entries 4i..4i+3 of
 * the DEVICE buffer tuples_dev (4 * n_overlaps tuples, 16-byte aligned) receive
 * (a, (a_begin+15)<<1), (a, (a_end-15)<<1|1), (b, ...), (b, ...); the read is RALA_HIP_NO_READ
 * for records that do not resolve.  The caller routes them to the read owners. */
int rala_hip_emit_bound_tuples(rala_hip_ctx* ctx, uint64_t* tuples_dev);
/* The same tuples grouped by owner rank (owner = read % world, stored read = read / world =
 * the owner's local read number): the device buffer receives the bucket of rank 0, then rank 1,
 * ...; counts[world] (host) receives the bucket sizes.  Records that do not resolve are left
 * out. */
int rala_hip_emit_bound_tuples_bucketed(rala_hip_ctx* ctx, uint32_t world, uint64_t* tuples_dev, uint64_t* counts);
/* Feed a context whose reads are the locally owned ones with the tuples it received (read =
 * LOCAL read number; other values are ignored).  rala_hip_initialize then skips duplicate
 * removal and builds / annotates the piles from these bounds. */
int rala_hip_set_bound_tuples(rala_hip_ctx* ctx, const uint64_t* tuples, uint64_t n, int mem);
/* Bound records: both bounds of one overlap side in ONE 8-byte element - local read (22 bits, as above) << 42 | begin (21
 * bits) << 21 | end (21 bits), the raw coordinates of src/graph.cpp:317-324 (the +-15 is applied by the owner);
 * coordinates of 2^21 - 1 and more are stored as 2^21 - 1 (outside every read the format is used for).  Half the bytes
 * of the all-to-all, and the owner buckets them through the partitioned path (csrc/bucket_kernels.hip).
 * rala_hip_bound_records_fit: 1 if every read is shorter than 2^21 - 32 bases and a rank owns fewer than 2^22 reads.
 * _emit_: as rala_hip_emit_bound_tuples_bucketed, one record per overlap side (2 * n_overlaps at most).
 * _set_: as rala_hip_set_bound_tuples. */
int rala_hip_bound_records_fit(const rala_hip_ctx* ctx, uint32_t world);
int rala_hip_emit_bound_records_bucketed(rala_hip_ctx* ctx, uint32_t world, uint64_t* records_dev, uint64_t* counts);
int rala_hip_set_bound_records(rala_hip_ctx* ctx, const uint64_t* records, uint64_t n, int mem);
/* Install the result of Graph::initialize computed elsewhere (gathered from the owners) into a
 * context that holds all reads and overlaps, so that rala_hip_construct can follow.  Host
 * arrays; interval CSR as returned by rala_hip_get_intervals (kinds 0 and 1). */
int rala_hip_import_state(rala_hip_ctx* ctx, const uint8_t* valid, const uint32_t* begin, const uint32_t* end,
                          const uint16_t* median, const uint16_t* p10, const uint8_t* alive,
                          const uint64_t* pits_off, const uint32_t* pits_pairs, const uint32_t* pits_aux,
                          const uint64_t* hills_off, const uint32_t* hills_pairs);

/* Device-resident view of the result of rala_hip_initialize, for device-to-device gathers:
 * per-read arrays of n_reads entries, the interval pool (12-byte {first, second, aux} records;
 * a read's pits, then its hills, start at slot[read], or slot == 0xFFFFFFFF) and the validity
 * bytes.  rala_hip_get_device_state fills the view from a context;
 * rala_hip_import_state_device installs a (gathered) view into a context that holds all
 * reads and overlaps, like rala_hip_import_state does from host arrays. */
typedef struct rala_hip_device_state {
    const uint32_t* begin;
    const uint32_t* end;
    const uint16_t* median;
    const uint16_t* p10;
    const uint8_t* alive;
    const uint32_t* n_pits;     /* 32-bit counts: the reference's lists are vectors (pile.hpp:164-169) */
    const uint32_t* n_hills;
    const uint32_t* slot;
    const void* pool;
    uint64_t pool_count;
    const uint8_t* valid;       /* may be NULL in a tuple-fed context */
} rala_hip_device_state;
int rala_hip_get_device_state(rala_hip_ctx* ctx, rala_hip_device_state* out);
/* Copy the context's arrays into the caller's device buffers (non-NULL members of dst;
 * dst->pool_count = capacity of dst->pool in records).  Lets a caller that owns its device
 * memory (a torch tensor handed to RCCL) avoid aliasing the context's buffers. */
int rala_hip_copy_device_state(rala_hip_ctx* ctx, const rala_hip_device_state* dst);
int rala_hip_import_state_device(rala_hip_ctx* ctx, const rala_hip_device_state* in);

/* ---- sharded run over the GPUs of one node --------------------------------------------------
 * The reference fans its per-pile work out over a thread pool (src/graph.cpp:235, :367-377,
 * :387-407, ...); here reads are partitioned over P GPUs (owner(read) = read % P), the overlap
 * file is cut into P slices on a_id-run boundaries (rala_hip_mg_slice_cuts), and ONE all-to-all
 * of 8-byte bound tuples over xGMI ships every bound to the owner of its read.  Everything that
 * is per overlap (duplicate removal, bound emission, trim / type, liveness, hill counters) runs on
 * the slice; everything that is per read (piles, annotation) on the owner; the in-order
 * containment scan is a fixed point whose bounds are all-reduced (min) per round; the survivors
 * (about 1 % of the overlaps) are all-gathered and the preprocess tail, the graph and the
 * transitive reduction run replicated on them.
 *
 * One rala_hip_mg object per rank.  Ranks are either processes (one per GPU, RCCL: rank 0 obtains
 * a 128-byte id with rala_hip_mg_unique_id and ships it to the others by any means) or host
 * threads of one process (RCCL with an id made in that process, or the in-process transport
 * RALA_HIP_COMM_LOCAL, which also lets several ranks share one device - how the decomposition
 * is tested on a single GPU).  rala_hip_mg_create and rala_hip_mg_run are collective: every rank
 * calls them.  After a run, rala_hip_mg_context(mg) holds the replicated result: all getters
 * of this header work on it, except rala_hip_get_pile_data (the coverage of read r lives on
 * rank r % P: rala_hip_mg_get_pile_data). */
enum { RALA_HIP_COMM_RCCL = 0, RALA_HIP_COMM_LOCAL = 1 };
typedef struct rala_hip_mg rala_hip_mg;
typedef struct rala_hip_mg_timings {
    /* wall-clock milliseconds of this rank's last run, by step */
    float emit_ms, exchange_ms, owner_ms, gather_ms, construct_ms, repeats_ms, tr_ms, total_ms;
    uint64_t tuples_sent;       /* bound tuples this rank shipped to other ranks */
} rala_hip_mg_timings;
int rala_hip_mg_unique_id(void* id128);
int rala_hip_mg_local_group_create(uint32_t world, void** group);
void rala_hip_mg_local_group_destroy(void* group);
/* token: the 128-byte id (RALA_HIP_COMM_RCCL) or the group (RALA_HIP_COMM_LOCAL) */
int rala_hip_mg_create(int device, uint32_t rank, uint32_t world, int transport, const void* token, rala_hip_mg** out);
/* The same in two steps: the rank's device contexts (NOT collective), then joining the group (collective: ncclCommInitRank).
 * A launcher creates all contexts first, makes sure every rank has its own, and only then lets them join - a rank that
 * failed before the collective part would leave the others waiting inside it. */
int rala_hip_mg_create_contexts(int device, uint32_t rank, uint32_t world, rala_hip_mg** out);
int rala_hip_mg_join(rala_hip_mg* mg, int transport, const void* token);
void rala_hip_mg_destroy(rala_hip_mg* mg);
const char* rala_hip_mg_last_error(const rala_hip_mg* mg);
/* all read lengths, on every rank (src/graph.cpp:249-264) */
int rala_hip_mg_set_reads(rala_hip_mg* mg, const uint32_t* read_len, uint64_t n_reads);
/* cuts[world + 1]: slice k = records cuts[k] .. cuts[k + 1] of the file; a cut never splits a run of
 * equal a_id, and records that do not resolve (query or target RALA_HIP_NO_READ) do not break a run
 * (src/graph.cpp:338-350).  b_id may be NULL when every target is known. */
int rala_hip_mg_slice_cuts(const uint32_t* a_id, const uint32_t* b_id, uint64_t n, uint32_t world, uint64_t* cuts);
/* this rank's slice; first = file position of its record 0 */
int rala_hip_mg_set_overlaps(rala_hip_mg* mg, const rala_hip_overlaps* slice, uint64_t n, uint64_t first, int mem);
/* The same from PAF TEXT (an uncompressed file), collective: rank k ships bytes [n k / P, n (k + 1) / P) of the file to its own
 * GPU and tokenises the lines that start there (rala_hip_set_overlaps_from_paf's kernels; the name table and the reads must be
 * set on rala_hip_mg_context(mg)); the ranks exchange their row counts and the queries at their ends, compute the same cuts
 * between runs of equal queries (rala_hip_mg_slice_cuts' rule) and move the rows in front of the cuts to the rank that holds
 * the run's start.  Replaces, for N GPUs, bioparser's parser in front of Graph::initialize (src/graph.cpp:328-382).
 * *length_error_read, *irregular: as rala_hip_set_overlaps_from_paf (the same values on every rank). */
int rala_hip_mg_set_overlaps_from_paf(rala_hip_mg* mg, const char* path, int check_lengths, uint32_t threads, int64_t* length_error_read,
                                      int* irregular);
/* An MHAP file the same way (src/graph.cpp:328-382; twelve numeric columns, no name table).
 * Both take a BGZF file too when the option "bgzf_in_pieces" is set on rala_hip_mg_context(mg) (default 0: a compressed file
 * is read as the text it is not, and is irregular): rank k takes the piece of its byte range (rala_hip_bgzf_index_range),
 * begin, end and emptiness of the pieces travel with the ranks' exchange, and a file whose pieces are not one chain
 * (rala_hip_bgzf_pieces_chain), a member the inflater refuses on any rank (CRC32, ISIZE) or a gzip file that is not BGZF is
 * *irregular = 8 on every rank, nothing set. */
int rala_hip_mg_set_overlaps_from_mhap(rala_hip_mg* mg, const char* path, int check_lengths, uint32_t threads, int64_t* length_error_read,
                                       int* irregular);
/* ---- a single-member gzip file that is not BGZF, over the ranks (option "gzip_in_pieces" beside "gzip_on_device") --------------
 * What gzip, pigz and `minimap2 | gzip` write.  With both options set on rala_hip_mg_context(mg) of EVERY rank (default 0: such a
 * file is *irregular = 8 on every rank before anything is shipped), rala_hip_mg_set_overlaps_from_paf / _mhap take it together.
 * The options are part of the collective call's contract - every rank makes the same calls in the same order with the same
 * options; ranks that differ wait for each other in exchanges the others do not make.
 * Every rank ships the whole compressed file and looks for block starts in its own chunks of "gzip_chunk_bytes" (rank k of P:
 * chunks [n k / P, n (k + 1) / P), chunk 0 always rank 0's); the ranks exchange the chunks' starts, count their own chunks -
 * each landing on a start some rank found - exchange the spans and build the same chain (rala_hip_gzip_chain).  A rank owns
 * the chain's jobs that begin in its chunks (rala_hip_gzip_pieces) and decodes them, and what the tokeniser's halo needs behind
 * them, into 16-bit symbols behind 32 768 markers "byte i of the 32 768 in front of this piece" - without a byte of the text in
 * front of it.  A kernel follows the markers of the last 32 768 symbols of its own text to bytes or to markers into the
 * window in front of the piece (the rank's OUT-window); the ranks exchange those 64 KB each and every rank composes the window
 * in front of its own piece from the ones of the ranks before it (rala_hip_gzip_compose_windows).  With that as the carry the
 * text is resolved as a window of a single context's walk is, the lines whose first byte lies in the rank's own text are
 * tokenised, and the CRC registers of the ranks' own texts, chained in rank order, must give the trailer's CRC32 (ISIZE and
 * the final block's end: the chain's).  Anything else - on any rank - is *irregular = 8 on every rank with nothing set; a
 * failure of one rank alone (device memory for its piece: symbols and text, 3 bytes per byte of text, are held at once) is
 * learned by every rank in the next exchange: every rank's call fails, and the group stays usable.
 * Not taken so, as before: BGZF (option "bgzf_in_pieces"), files of several members (unless "gzip_members" is set too, below); -s files
 * have an entry of their own (rala_hip_mg_tokenise_sensitive, below).
 *
 * The split of a chain over the parts (no context, no device): job j begins at bit job_start_bit[j] (ascending) of a file whose
 * deflate bytes begin at deflate_off and are cut into n_chunks chunks of chunk_bytes; part k's jobs are
 * [first_job[k], first_job[k + 1]) - first_job has parts + 1 entries, an empty run is legal.  RALA_HIP_EINVAL: parts or
 * chunk_bytes 0, jobs without chunks, a first bit in front of deflate_off, starts that do not ascend. */
int rala_hip_gzip_pieces(const uint64_t* job_start_bit, uint64_t n_jobs, uint64_t deflate_off, uint64_t chunk_bytes, uint64_t n_chunks,
                         uint32_t parts, uint64_t* first_job);
/* The window in front of part `part` (< parts) from the parts' out-windows (no context, no device).  out_windows[r * 32768 + i]:
 * the symbol 32 768 - i in front of the end of part r's own text - a byte (< 0x100), or 0x8000 | k: entry k of the window in
 * front of part r (0x8000 | 0 is such a marker).  W_0 is nothing at all; W_{r+1}[i] = out_r[i] where that is a byte, else
 * W_r[out_r[i] & 0x7FFF].  in_window[i] = W_part[i]: a byte, or RALA_HIP_GZIP_NOTHING where the file's text has not begun
 * (the carry the device gets says 0x8000 there, the convention of its kernels).  *valid = 0: an entry that is neither byte nor
 * marker, or nothing BEHIND a byte - a window is the tail of the text, so nothing stands in front of all its bytes or a match
 * copied it from in front of the file's first byte, which zlib refuses. */
#define RALA_HIP_GZIP_NOTHING 0x4000
int rala_hip_gzip_compose_windows(const uint16_t* out_windows, uint32_t parts, uint32_t part, uint16_t* in_window, int* valid);
/* the rank's piece in the last rala_hip_mg_set_overlaps_from_paf / _mhap on the slice context: every such call begins with zeros,
 * and zeros stay where the file was not taken together (options off, another kind of file) or was refused before the resolve */
typedef struct rala_hip_gzip_pieces_info {
    uint64_t own_chunks;            /* chunks the rank looked for a start in and counted */
    uint64_t own_jobs;              /* jobs of the chain that begin in them */
    uint64_t halo_jobs;             /* jobs behind them decoded for the tokeniser's halo */
    uint64_t own_text_bytes;
    uint64_t window_markers;        /* own symbols that resolved through the composed window in front of the piece */
    uint32_t longest_chase;         /* the compose kernel's longest way from a symbol to a byte or to that window, in hops */
    float compose_ms;               /* the compose kernel and its copies */
    float exchange_ms;              /* the four host exchanges, waiting for the slowest rank included */
} rala_hip_gzip_pieces_info;
int rala_hip_get_gzip_pieces_info(rala_hip_ctx* ctx, rala_hip_gzip_pieces_info* out);
/* ---- a gzip file of SEVERAL members that is not BGZF, over the ranks ("gzip_members" beside the two options above) --------------
 * cat part*.paf.gz, pigz -i.  With "gzip_on_device", "gzip_in_pieces" and "gzip_members" set on rala_hip_mg_context(mg) of EVERY
 * rank, rala_hip_mg_set_overlaps_from_paf / _mhap take such a file together (one member included); "gzip_members" is compared in
 * the first exchange, ranks that disagree on it all return RALA_HIP_EINVAL and the group stays usable.  Every rank finds the member
 * headers of the whole file (the list is exact, the same everywhere), counts those whose deflate bytes begin in its own chunks
 * from their first block as from a stream's first chunk, and the spans travel with the chunks'; every rank walks the same words
 * (rala_hip_gzip_chain_members): the same jobs, members and verdict everywhere, and where a member begins is never guessed from
 * a byte range.  Jobs are owned as before; a member's first job emits no markers and every later one carries its member's floor.
 * The out-window's chase ends at the floor of the member its first symbol belongs to (a hop below it: nothing, flag 8); the
 * window in front of a piece is composed as before and masked in front of the member the piece begins in
 * (rala_hip_gzip_compose_windows_masked).  Every member is proven alone: ISIZE in the chain, CRC32 against ITS trailer - inside
 * one rank's text by that rank, across ranks from at most two partial registers per rank that ride on the last exchange
 * (rala_hip_gzip_members_proof).  Anything else is *irregular = 8 on every rank with nothing set.
 * rala_hip_get_gzip_members on every rank's slice context gives the file's members, the same on every rank.
 *
 * The masked composition (no context, no device): reach[r], r < parts = the text bytes between the first byte of the member in
 * which part r's text begins and part r's first byte, clamped to 32 768.  in_window = the window in front of `part` as
 * rala_hip_gzip_compose_windows gives it with every entry more than reach[part] in front of the part RALA_HIP_GZIP_NOTHING;
 * *before = the byte in front of the part from the UNMASKED window (lines straddle members), -1: the text begins with the part;
 * *valid = 0: what rala_hip_gzip_compose_windows refuses, or an entry within reach[r] of a part r <= part that is no byte. */
int rala_hip_gzip_compose_windows_masked(const uint16_t* out_windows, uint32_t parts, const uint64_t* reach, uint32_t part, uint16_t* in_window,
                                         int* before, int* valid);
/* The members' proof over parts (no context, no device).  Part p holds the text [part_begin[p], part_end[p]), the parts in order
 * and back to back from 0 to the text's end.  A part owes: local_bad[p] = the first member that lies inside its text alone and is
 * not its trailer's (~0: none); {head_reg, head_len}[p] = CRC register (from zero, no final inversion: rala_hip_crc32_chain's
 * convention) and length of its first bytes where they belong to a member begun in front of it; {tail_reg, tail_len}[p] = the
 * same of its last bytes where they belong to a member begun in it that goes on behind it; zeros where there is no such member.
 * A member that spans parts is the chain of those registers in part order against member_crc32; an empty member's CRC32 is 0.
 * *valid = 0 with *bad_member = the first member that fails (n_members: the parts are not the members' text). */
int rala_hip_gzip_members_proof(const uint64_t* member_text_off, const uint64_t* member_text_n, const uint32_t* member_crc32, uint64_t n_members,
                                const uint64_t* part_begin, const uint64_t* part_end, const uint32_t* head_reg, const uint64_t* head_len,
                                const uint32_t* tail_reg, const uint64_t* tail_len, const uint64_t* local_bad, uint32_t parts, uint64_t* bad_member,
                                int* valid);
/* what the rank's piece saw of the members in the last such call on the slice context (zeros otherwise) */
typedef struct rala_hip_gzip_member_pieces_info {
    uint64_t own_candidates;        /* member headers whose deflate bytes begin in the rank's chunks: counted by it */
    uint64_t members_begun;         /* members (not empty) whose first byte lies in its own text */
    uint64_t member_ends;           /* members (not empty) whose last byte lies in its own text: where its range is cut for the proof */
    uint32_t registers_sent;        /* partial CRC registers it gave for members that span ranks: 0 - 2 */
    uint32_t floor_stops;           /* chases gzip_window_compose_members_kernel ended at a member's floor (each one refuses the file) */
    float compose_ms;               /* that kernel and its copies */
    float pad;
} rala_hip_gzip_member_pieces_info;
int rala_hip_get_gzip_member_pieces_info(rala_hip_ctx* ctx, rala_hip_gzip_member_pieces_info* out);
/* The -s file of a sharded run through ONE collective (every rank calls it, with the same options on its slice context): rank k's
 * share of the sensitive overlaps tokenised on its GPU into the buffers rala_hip_tokenise_sensitive uses - never into the primary
 * overlaps' columns -, no length check.  format 0: PAF, 1: MHAP.  Plain text and BGZF: the rank's part as
 * rala_hip_tokenise_sensitive(ctx, path, format, rank, world, ..) takes it, the BGZF pieces' begin, end and emptiness exchanged and
 * joined on every rank - the caller has nothing to join.  A gzip file that is not BGZF, of one member ("gzip_on_device" +
 * "gzip_in_pieces") or of several (+ "gzip_members"): taken together as rala_hip_mg_set_overlaps_from_paf takes it, without cuts -
 * a rank's share is the lines whose first byte lies in its own text (any contiguous shares will do for rala_hip_mg_run).
 * out: device pointers that stay the slice context's, for rala_hip_mg_run with "sensitive_in_device_memory"; compressed bytes,
 * symbols and text are released before it returns.  *irregular (flag 8: a file that cannot be proven), a failure of any rank
 * (RALA_HIP_ENOMEM there, RALA_HIP_EDEVICE elsewhere) and RALA_HIP_ETOOLARGE are every rank's verdict, and the group stays usable. */
int rala_hip_mg_tokenise_sensitive(rala_hip_mg* mg, const char* path, int format, uint32_t threads, rala_hip_overlaps* out, uint64_t* n,
                                   int* irregular);
/* the rank's slice as it was set: file position of its record 0, records (the columns: rala_hip_get_overlap_columns on
 * rala_hip_mg_context(mg)) */
int rala_hip_mg_get_slice(rala_hip_mg* mg, uint64_t* first, uint64_t* n);
/* Graph::construct + remove_transitive_edges (src/graph.cpp:427-640, :1281-1335); sens_slice = this
 * rank's share of the sensitive overlaps (any contiguous share, n_sens = 0 allowed; NULL on EVERY
 * rank for a run without them - ranks that disagree get RALA_HIP_EINVAL).  A failure of one rank
 * alone (out of memory, a device error) aborts the group: every rank's call fails and the rank
 * objects must be destroyed. */
int rala_hip_mg_run(rala_hip_mg* mg, const rala_hip_overlaps* sens_slice, uint64_t n_sens, uint32_t* n_pairs);
/* the same for n ranks of this process, one host thread per rank, joined before it returns */
int rala_hip_mg_run_threads(rala_hip_mg** ranks, uint32_t n, const rala_hip_overlaps* sens_slices, const uint64_t* n_sens,
                            uint32_t* n_pairs);
rala_hip_ctx* rala_hip_mg_context(rala_hip_mg* mg);
/* the context of the reads this rank owns (local read j = read j * P + rank): stage timings of the pile kernels */
rala_hip_ctx* rala_hip_mg_owner_context(rala_hip_mg* mg);
int rala_hip_mg_get_pile_data(rala_hip_mg* mg, uint64_t read, uint16_t* data);
/* rala_hip_get_pile_row_digests (below) of the rows this rank owns: n_owned = the reads r with r % P == rank, entry j = read
 * j * P + rank, under the final valid regions */
int rala_hip_mg_get_pile_row_digests(rala_hip_mg* mg, uint64_t* fnv, uint64_t* inside, uint64_t* outside);
int rala_hip_mg_get_timings(rala_hip_mg* mg, rala_hip_mg_timings* out);

/* Force-directed layout of one connected component, the O(n^2) part of Graph::postprocess
 * (src/graph.cpp:1132-1226): n points x, y (host, in / out); the attraction partners of point
 * i are adj[adj_off[i] .. adj_off[i + 1]) (point indices, n = a point fixed at the origin: a
 * neighbour outside the component); `iterations` steps with step length t, decreased by dt
 * after every step, spring constant k.  Same arithmetic, in the same order, as the reference's
 * per-point task. */
int rala_hip_layout(rala_hip_ctx* ctx, uint32_t n, double* x, double* y, const uint32_t* adj_off, const uint32_t* adj,
                    uint32_t iterations, double k, double t, double dt);

/* The same for all components of a round in one call (src/graph.cpp:1132-1226 once per component of the loop at :1106): the
 * result equals rala_hip_layout on every component's slice in turn, bit for bit; components do not interact.  The points of
 * component c are x / y[comp_off[c] .. comp_off[c + 1]) (host, in / out, component after component); the partners of point p
 * (an index into the concatenation) are adj[adj_off[p] .. adj_off[p + 1]), as COMPONENT-LOCAL point indices, n_c = the origin
 * as above; k[c] is the component's spring constant; iterations, t and dt are shared.  One upload, the device work, one
 * download, one wait.  A component of at most "layout_fused_max" points (rala_hip_set_option) is laid out by one workgroup
 * that keeps the positions in LDS through all steps - one launch per size class (256 / 1024 points) over all such components;
 * the larger ones take one launch per step together.
 * Checked on the host before anything is enqueued (RALA_HIP_EINVAL, nothing touched): comp_off and adj_off start at 0 and do
 * not decrease, every adj value of component c is at most n_c.  Empty components, n_components == 0 and iterations == 0 are
 * valid and leave x and y as they are. */
int rala_hip_layout_batch(rala_hip_ctx* ctx, uint32_t n_components, const uint32_t* comp_off, double* x, double* y,
                          const uint32_t* adj_off, const uint32_t* adj, const double* k, uint32_t iterations, double t,
                          double dt);
/* The last rala_hip_layout_batch of the context (zeros before the first; a refused call leaves the previous one's). */
typedef struct rala_hip_layout_info {
    uint32_t components_fused_256, components_fused_1024;   /* one workgroup of 256 / 1024 threads each, all steps in one launch */
    uint32_t components_stepped;                            /* larger ones: one launch per step for all of them */
    uint32_t components_empty;
    uint64_t points_fused_256, points_fused_1024, points_stepped;
    uint32_t step_tiles;        /* workgroups of one step launch */
    uint32_t launches;          /* kernel launches enqueued */
    float device_ms;            /* between two HIP events around the kernels (without the copies) */
} rala_hip_layout_info;
int rala_hip_get_layout_info(rala_hip_ctx* ctx, rala_hip_layout_info* out);

/* ---- the layout of a round's components shared by the ranks of a sharded run --------------------------------------------------
 * A step is a Jacobi step: every point's new position depends on the previous positions only, so any split of the POINTS over the
 * ranks gives the bits of rala_hip_layout_batch.  What travels per step is 16 bytes per point against n_c pair terms per point.
 *
 * The split (no context, no device).  Units, in point order, component after component: a component of at most fused_max points
 * is ONE unit of cost n_c^2 (one workgroup runs all its steps: it stays whole); a larger one is its tiles of 256 points, each of
 * cost (points in the tile) * n_c; an empty component is no unit.  Part k ends behind the first unit at which the cost of the
 * units up to and including it reaches ceil(total * (k + 1) / parts); the last part ends at N = comp_off[n_components].  Part k is
 * the points [first_point[k], first_point[k + 1]) - first_point has parts + 1 entries, an empty part is legal - and cost[k]
 * (parts entries, may be NULL) the cost of its units: at most ceil(total / parts) + the largest unit's cost.
 * RALA_HIP_EINVAL: parts == 0, first_point or (with components) comp_off NULL, a comp_off that does not start at 0 or decreases,
 * fused_max > 1024. */
int rala_hip_layout_split(uint32_t n_components, const uint32_t* comp_off, uint32_t fused_max, uint32_t parts,
                          uint32_t* first_point, uint64_t* cost);
/* rala_hip_layout_batch by all ranks of a group together (collective: every rank calls it with the SAME inputs, as for
 * rala_hip_mg_run; x and y are inputs here, the result goes to x_out / y_out, which may be x / y).  "layout_fused_max" is read
 * from rala_hip_mg_context(mg) and must be equal on all ranks (compared in the call's one host exchange: ranks that differ all
 * get RALA_HIP_EINVAL, the group stays usable).  The host checks are those of rala_hip_layout_batch, made before anything is
 * enqueued or exchanged (RALA_HIP_EINVAL; the same inputs give the same verdict on every rank, so nobody waits for a rank that
 * refused); no components, no points and iterations == 0 are valid, touch nothing and make no exchange.
 * Every rank uploads the whole batch (positions as {x, y} pairs, offsets, partner lists, k, the tile table), takes part `rank`
 * of rala_hip_layout_split over `world` parts, runs its fused components in one launch per size class and, per step, its range
 * of the tile table (layout_shard_step_kernel) followed by ONE all-gather of the ranks' point ranges of the buffer just written
 * (in place; the last one carries the fused results too; without any tile one gather behind the fused launches takes its
 * place).  A rank whose x_out and y_out are both NULL takes part without a download.
 * A device error or RALA_HIP_ENOMEM on one rank alone behaves as in rala_hip_mg_run: the rank aborts the group, every rank's
 * call fails and the rank objects are to be destroyed.  RCCL: never run with a peer; tested with the in-process transport. */
int rala_hip_mg_layout_batch(rala_hip_mg* mg, uint32_t n_components, const uint32_t* comp_off, const double* x, const double* y,
                             double* x_out, double* y_out, const uint32_t* adj_off, const uint32_t* adj, const double* k,
                             uint32_t iterations, double t, double dt);
/* the same for n ranks of this process, one host thread per rank, joined before it returns: rank 0 downloads into the caller's
 * x / y (in / out), the others pass NULL */
int rala_hip_mg_layout_batch_threads(rala_hip_mg** ranks, uint32_t n, uint32_t n_components, const uint32_t* comp_off, double* x,
                                     double* y, const uint32_t* adj_off, const uint32_t* adj, const double* k, uint32_t iterations,
                                     double t, double dt);
/* The rank's share of its last rala_hip_mg_layout_batch (zeros before the first; a refused call leaves the previous one's). */
typedef struct rala_hip_mg_layout_info {
    uint32_t first_point, end_point;                        /* the rank's points: [first_point, end_point) of the batch */
    uint32_t components_fused_256, components_fused_1024;   /* its fused components per size class */
    uint32_t step_tiles;        /* its tiles: workgroups of one of its step launches */
    uint32_t launches;          /* kernel launches it enqueued */
    uint32_t gathers;           /* all-gathers it took part in */
    uint64_t cost;              /* its part's cost (rala_hip_layout_split) */
    uint64_t total_cost;        /* all parts' */
    uint64_t bytes_received;    /* positions of other ranks' points, all gathers */
    float device_ms;            /* between two HIP events around its kernels, summed over the steps (without copies and gathers) */
    float exchange_ms;          /* wall clock inside the gathers: waiting for the slowest rank included */
} rala_hip_mg_layout_info;
int rala_hip_mg_get_layout_info(rala_hip_mg* mg, rala_hip_mg_layout_info* out);

/* ---- results (host buffers owned by the caller) --------------------------------------- */
/* is_valid_overlap_ (src/graph.hpp:168), one byte per overlap */
int rala_hip_get_valid(rala_hip_ctx* ctx, uint8_t* valid);
/* Pile::begin/end/median/p10 and liveness (piles_[i] != nullptr) of every read, as they
 * stand after the last completed stage.  Any pointer may be NULL. */
int rala_hip_get_piles(rala_hip_ctx* ctx, uint32_t* begin, uint32_t* end, uint16_t* median, uint16_t* p10,
                       uint8_t* alive);
/* Pile::data() of one read (src/pile.hpp:53): read_len[read] values.  Contents are
 * defined for reads that passed find_valid_region. */
int rala_hip_get_pile_data(rala_hip_ctx* ctx, uint64_t read, uint16_t* data);
/* Checksums of EVERY pile row where it lies in device memory (Pile::data() of all reads is 20 GB at 1 M reads: nothing a
 * caller wants copied), n_reads entries each, any pointer may be NULL: fnv[r] = FNV-1a-64 over the bytes of Pile::data() of
 * read r (src/pile.hpp:53: uint16 values, low byte first, zero outside the valid region as Pile::shrink leaves them,
 * src/pile.cpp:311-318) - what rala_hip_get_pile_data would return, hashed on the device; inside[r] = the sum of the row over
 * [begin, end); outside[r] = the sum of the values STORED outside it (zero right after rala_hip_initialize; later stages narrow a
 * region without rewriting its row).  A filtered read answers 0 to all three. */
int rala_hip_get_pile_row_digests(rala_hip_ctx* ctx, uint64_t* fnv, uint64_t* inside, uint64_t* outside);
/* Where the rows are (option "pile_rows"; either pointer may be NULL).  resident_bytes: the size of the rows' allocation - at least
 * 2 bytes per base of all reads with pile_rows = 1, 0 with pile_rows = 0.  rows_materialised: rows rebuilt from their events since
 * the last rala_hip_initialize (always 0 with pile_rows = 1).
 * With pile_rows = 0: rala_hip_get_pile_data rebuilds the one row; rala_hip_get_pile_row_digests walks all reads in batches of
 * "pile_rows_scratch_mb" and hashes every batch where it was rebuilt - fnv and inside are what the resident rows give, outside is 0
 * by definition (nothing is stored, so nothing is stored outside a region); the rala_hip_mg_ twins do the same on the owner
 * contexts (rala_hip_mg_owner_context takes the options).  A rebuilt row is Pile::add_layers over the primary bounds and, after a
 * construct with sensitive overlaps, a second one over the sensitive bounds of the targets: those bounds are kept until the next
 * rala_hip_initialize (of a construct that failed they are not used), and rala_hip_construct refuses a second set of sensitive
 * overlaps after one that succeeded on the same rala_hip_initialize (RALA_HIP_EINVAL) - where the rows are resident its layers
 * would pile up on the first one's, here they would replace them; a sharded run initializes every time.  "debug_pile_stop_after"
 * other than 99 is refused by rala_hip_initialize in this mode. */
int rala_hip_get_pile_rows_info(rala_hip_ctx* ctx, uint64_t* resident_bytes, uint64_t* rows_materialised);
/* Pits / hills / repeat hills of all reads as CSR: offsets[n_reads + 1], then pairs
 * (first, second) and one aux word per interval (pit: min coverage inside; hill:
 * spanning-overlap count; repeat hill: bridged flag).  kind: 0 pits, 1 hills, 2 repeat
 * hills.  Call with pairs = NULL to obtain offsets only. */
int rala_hip_get_intervals(rala_hip_ctx* ctx, int kind, uint64_t* offsets, uint32_t* pairs, uint32_t* aux);
/* Overlaps kept for the graph (which = 0) or as internals (which = 1) after construct.
 * Returns the count through *n; arrays may be NULL to query the count. */
int rala_hip_get_overlaps(rala_hip_ctx* ctx, int which, uint64_t* n, uint32_t* src_index, uint32_t* a_begin,
                          uint32_t* a_end, uint32_t* b_begin, uint32_t* b_end, uint32_t* length, uint8_t* type);
/* Assembly graph: node k belongs to read node_read[k] (k odd = reverse complement);
 * edges in id order with twin e^1; marks as set by rala_hip_remove_transitive_edges. */
int rala_hip_get_graph_size(rala_hip_ctx* ctx, uint64_t* n_nodes, uint64_t* n_edges);
int rala_hip_get_graph(rala_hip_ctx* ctx, uint32_t* node_read, uint32_t* src, uint32_t* dst, uint32_t* len,
                       uint8_t* marks);
int rala_hip_get_timings(rala_hip_ctx* ctx, rala_hip_timings* out);
/* number of reads dropped by find_valid_region (src/graph.cpp:409-424) */
int rala_hip_get_num_prefiltered(rala_hip_ctx* ctx, uint64_t* n);

#ifdef __cplusplus
}
#endif

#endif /* RALA_HIP_H_ */
