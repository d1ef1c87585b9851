// Stage functions of librala_hip shared by the single-GPU entry points (the stage files; what only those share: orchestration.h) and the
// sharded runner (sharded.hip).  A non-null Comm makes a stage collective: every rank of the
// group calls it with its own slice of the overlaps and the same per-read state.
#pragma once

#include "comm.h"
#include "context.h"

namespace rala_hip {

// second overlap pass (graph.cpp:443-518) .. Graph::preprocess for chimeras (:699-880) .. node and
// edge construction (:553-632) on ctx->ovl (file positions ctx->ovl.base + i):
//   classify (trim / type, killer list)                      per overlap of the slice
//   containment fixed point                                  comm: bounds all-reduced (min) per round
//   liveness, hill counters, survivors                       comm: counters all-reduced (sum),
//                                                                  survivor lists all-gathered
//   preprocess tail + graph on the survivors                 replicated
int construct_stages(rala_hip_ctx* ctx, Comm* comm, bool sensitive_pass_follows = false);

// Graph::preprocess with the sensitive overlaps (graph.cpp:882-1054) behind construct_stages:
// cs = the context construct_stages ran on, with this rank's share of the sensitive overlaps;
// cl = the context that holds the piles (the same one on a single GPU, comm = null)
int repeats_stage(rala_hip_ctx* cs, rala_hip_ctx* cl, Comm* comm, const rala_hip_overlaps* sens, uint64_t n_sens);

// Graph::remove_transitive_edges (graph.cpp:1281-1335) on the graph construct_stages left on the
// device; with a communicator every rank probes from its share of the edges and the marks are
// all-reduced
int transitive_stage(rala_hip_ctx* ctx, Comm* comm, uint32_t* n_pairs);

// install per-read state that was computed elsewhere and already sits in ctx's device arrays
// (d_begin .. d_iv_slot, d_pool[0 .. pool_count)); validity bits of ctx's own overlaps must be
// there too (rala_hip_dedupe).  Counts the filtered reads.
int install_read_state(rala_hip_ctx* ctx, uint64_t pool_count);

// sharded runs, the bounds scattered once on the sender (bucket_kernels.hip): the sender's and the owner's side
int shard_emit(rala_hip_ctx* ctx, const ShardGeometry& g, uint64_t* send, uint64_t* words);
int set_bound_blocks(rala_hip_ctx* ctx, const uint64_t* base, const uint64_t* base_self, const ShardBlocks& blocks, const ShardGeometry& g,
                     uint64_t n_records);

// the device tokeniser (ingest.hip): the lines that start in bytes [lo, hi) of a PAF file into the target's columns
struct PafTarget {
    DevBuf<uint32_t>* col[7];       // a_id, b_id, a_begin, a_end, b_begin, b_end, length
    DevBuf<uint8_t>* strand;
    bool mhap = false;              // the file is MHAP: twelve blank-separated numeric columns, no names
};
struct PafRange {
    uint64_t n_lines = 0;
    unsigned long long first_bad = ~0ull;      // row << 32 | read of the first record whose length differs from its sequence's
    uint32_t flags = 0;                        // != 0: not a file of 12-column records (kernels.h: launch_paf_parse)
    uint64_t file_bytes = 0;
};
int paf_tokenise_range(rala_hip_ctx* ctx, const char* path, uint64_t lo, uint64_t hi, bool check_lengths, uint32_t threads,
                       size_t extra_rows, const PafTarget& T, PafRange* out);

// Part `part` of `parts` of an overlap file of whatever kind, by BYTES OF THE FILE (part k covers [F / P k + min(k, F % P), ...),
// the split of the sharded ingest): a plain file gives the lines that start in the part's bytes, exactly as
// paf_tokenise_range; a BGZF file (take.bgzf_pieces) the part's piece - the members whose header begins in its bytes,
// indexed, shipped and inflated without a look at anything in front of them, the lines whose first byte follows a byte of
// the piece's text (the line at text offset 0: part 0's); any other gzip file (take.gzip_whole, parts == 1, the context's
// option gzip_on_device) its whole text.  A compressed file that is not taken so: flags = 8 with take.refuse_other,
// otherwise read as the text it is not (the tokeniser's flags say so).  piece[0 .. 2] = begin, end, empty of the part
// (ingest_formats.h: BgzfPiece; a plain file: its byte range): the caller checks that the pieces join (bgzf_pieces_chain).
// The compressed bytes and the text are released before it returns.  *bgzf: the file was taken in pieces.
struct PartKinds {
    bool bgzf_pieces = false, gzip_whole = false, refuse_other = false;
};
int overlap_tokenise_part(rala_hip_ctx* ctx, const char* path, uint32_t part, uint32_t parts, const PartKinds& take, bool check_lengths,
                          uint32_t threads, size_t extra_rows, const PafTarget& T, PafRange* out, uint64_t piece[3], bool* bgzf);

// A single-member gzip overlap file that is not BGZF taken by the ranks of a sharded run TOGETHER (option gzip_in_pieces beside
// gzip_on_device; ingest_gzip.hip), as steps with a host exchange between each two of them (sharded.hip makes those: every rank
// makes every exchange, whatever a step returned).  `all` is what agree_with gathered: part p's words at all[p * stride + 1 ..].
//   open      the file opened, its header and trailer read (no device): head = {1 if it is such a file, file size, where the
//             deflate bytes begin, chunks, the (last) trailer's CRC32, its ISIZE, the option gzip_members} (7 words) - the ranks compare them before anything is shipped;
//   find      the file shipped, block starts found in the part's own chunks (ingest_formats.h: gzip_part_chunk), with gzip_members the
//             member headers of the whole file                     -> `most` + 1 words: the own chunks' starts, the headers found (or 0)
//   count     the own chunks counted, landing on the starts any rank found, with gzip_members the own header candidates too
//                                                                   -> gzip_piece_span_words: 4 per chunk and candidate of the most any part owns
//   write     the chain (the same on every rank from the same words; *valid = false: refused, the steps end here), the own jobs
//             and the halo's written, the out-window composed (gzip_window_compose_kernel)                       -> 8192 words
//   tokenise  the window in front of the piece composed from all out-windows and uploaded as the carry, windows and resolve as
//             they are, the lines that begin in the own text tokenised; own = {CRC register, length} of the own text
//   proven    the registers of all parts chained: the trailer's CRC32 and the text's size
//   close     the compressed bytes, symbols and text released, on every way out
// With the option gzip_members beside them a file of SEVERAL members is taken the same way (head[6] = the option, compared by the
// ranks): find also finds the member headers of the whole file (the same list on every rank; the last of its most + 1 words is
// their number), count also counts the candidates whose deflate bytes begin in the own chunks (gzip_piece_span_words: the words
// every part gives), write walks gzip_chain_members and composes the out-window with member floors
// (gzip_window_compose_members_kernel), tokenise masks the window in front of the member the piece begins in and proves the
// members inside the own text, own[2 .. 6] = what it owes the members that span ranks, members_proven: all of them, on every rank.
struct GzipPieceRun;
int gzip_piece_open(rala_hip_ctx* ctx, const char* path, bool mhap, uint64_t head[7], GzipPieceRun** run);
uint64_t gzip_piece_most_chunks(uint64_t n_chunks, uint32_t parts);
int gzip_piece_find(rala_hip_ctx* ctx, GzipPieceRun* g, uint32_t part, uint32_t parts, uint32_t threads, std::vector<uint64_t>& starts_out);
int gzip_piece_count(rala_hip_ctx* ctx, GzipPieceRun* g, const uint64_t* all, size_t stride, std::vector<uint64_t>& spans_out);
int gzip_piece_write(rala_hip_ctx* ctx, GzipPieceRun* g, const uint64_t* all, size_t stride, bool* valid, std::vector<uint64_t>& window_out);
int gzip_piece_resolve(rala_hip_ctx* ctx, GzipPieceRun* g, const uint64_t* all, size_t stride, uint32_t* flag, uint64_t own[7]);
void gzip_piece_text(const GzipPieceRun* g, uint64_t* own_n, uint64_t* n_w, uint64_t* file_n, float* ship_ms, uint32_t* n_readers);
int gzip_piece_tokenise(rala_hip_ctx* ctx, GzipPieceRun* g, const uint64_t* all, size_t stride, bool check_lengths, uint32_t threads,
                        size_t extra_rows, const PafTarget& T, PafRange* out, uint64_t own[7]);
bool gzip_piece_proven(const GzipPieceRun* g, const uint32_t* reg, const uint64_t* len, uint32_t parts);
size_t gzip_piece_span_words(GzipPieceRun* g, const uint64_t* all, size_t stride);
bool gzip_piece_members(const GzipPieceRun* g);
bool gzip_piece_members_proven(const GzipPieceRun* g, const uint64_t* all, size_t stride, size_t at);
void gzip_piece_exchange_ms(rala_hip_ctx* ctx, float ms);
void gzip_piece_close(rala_hip_ctx* ctx, GzipPieceRun* g);

// rala_hip_mg_layout_batch (layout_shard.hip), as steps with the caller's one host exchange between the first two (sharded.hip
// makes it: the status word and layout_fused_max):
//   check     the host checks of rala_hip_layout_batch (no device); *why names what was refused
//   prepare   the split for `world` parts, the rank's fused lists and tile range, the batch packed and its upload enqueued
//             (nothing collective: a failure here travels with the exchange)
//   steps     the fused launches, then per step the rank's tiles and one all-gather of the buffer just written; the download
//             (x_out and y_out both null: none).  A failure in here is the rank's alone.
struct LayoutShardBatch {
    uint32_t n_components;
    const uint32_t* comp_off;
    const double *x, *y;
    const uint32_t *adj_off, *adj;
    const double* k;
    uint32_t iterations;
    double t, dt;
};
struct LayoutShardState {
    DevBuf<unsigned char> d_block;
    PinnedBuf<unsigned char> p_block;
    hipEvent_t ev[2] = {};
    rala_hip_mg_layout_info info = {};
    // of the call under way (prepare -> steps)
    std::vector<uint32_t> first_point;
    uint32_t n_list256 = 0, n_list1024 = 0, tile_first = 0, n_tiles_all = 0;
    size_t o_k = 0, o_comp = 0, o_adj_off = 0, o_adj = 0, o_l256 = 0, o_l1024 = 0, o_tiles = 0, o_pos1 = 0;
};
int layout_shard_check(const LayoutShardBatch& b, const char** why);
int layout_shard_prepare(rala_hip_ctx* ctx, LayoutShardState& st, uint32_t rank, uint32_t world, const LayoutShardBatch& b);
int layout_shard_steps(rala_hip_ctx* ctx, Comm* comm, LayoutShardState& st, const LayoutShardBatch& b, double* x_out, double* y_out);
void layout_shard_release(LayoutShardState& st);

// checksums of the rows cl holds (verify_kernels.hip) under the regions / liveness given per row (host arrays, cl->n_reads entries)
int pile_row_digests(rala_hip_ctx* cl, const uint32_t* begin, const uint32_t* end, const uint8_t* alive, uint64_t* fnv, uint64_t* inside,
                     uint64_t* outside);

// the stored values of one row of cl to the host (nothing zeroed): copied from the resident rows, or - option pile_rows = 0 -
// rebuilt from the read's events (pile_rows_kernel.hip)
int pile_row_to_host(rala_hip_ctx* cl, uint64_t read, uint16_t* data);

hipError_t stream_sync(rala_hip_ctx* ctx, hipStream_t s);
hipError_t d2h_small(rala_hip_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s);
int flush_upload(rala_hip_ctx* ctx);       // (context.hip) RALA_HIP_MEM_HOST_ASYNC columns not uploaded yet: now
int download_read_state(rala_hip_ctx* ctx);     // (getters.hip) the per-read state into the host's vectors

}  // namespace rala_hip
