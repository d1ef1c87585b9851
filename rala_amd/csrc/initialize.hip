// librala_hip: the first stage - duplicate removal, the bound events bucketed by read, the pile chain.  Implements
// rala_hip_initialize, rala_hip_dedupe, rala_hip_emit_bound_tuples, rala_hip_emit_bound_tuples_bucketed,
// rala_hip_emit_bound_records_bucketed and rala_hip_bound_records_fit of rala_hip.h, and shard_emit of stages.h.
// rala_hip_initialize decides first (InitPlan, from the context's options and sizes; nothing is enqueued) and then runs the
// plan's steps; what does not fit - a fixed slot, the interval pool - makes the call run the attempt again.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>

#include "lifecycle.h"
#include "orchestration.h"

using namespace rala_hip;

namespace {

// What duplicate removal inside a counting pass needs (kernels.h: BucketDedupe): the list of the marked runs, two halves of
// kMarks entries in d_dedupe_list (the option debug_dedupe_list_cap makes tests overflow it), and a zeroed word that counts
// the marks - `count`, the caller's own, or (null) the word behind the list, which the caller then clears.  counted: the
// caller's event behind the counting pass.
int counted_dedupe(rala_hip_ctx* ctx, uint32_t* count, hipEvent_t counted, BucketDedupe& bd) {
    constexpr uint32_t kMarks = 1u << 20;           // (C3: 1 - 2 % of a million queries)
    HIPCHECK(ctx->d_dedupe_list.ensure(2 * (size_t)kMarks + 4));
    bd = BucketDedupe{};
    bd.suspect = ctx->d_suspect.p; bd.valid = ctx->d_valid.p; bd.list_pos = ctx->d_dedupe_list.p; bd.list_query = ctx->d_dedupe_list.p + kMarks;
    bd.list_cap = ctx->debug_dedupe_list_cap ? std::min(kMarks, ctx->debug_dedupe_list_cap) : kMarks;
    bd.list_count = count ? count : ctx->d_dedupe_list.p + 2 * (size_t)kMarks;
    bd.counted = counted;
    return RALA_HIP_OK;
}

// ---- the plan of one attempt ------------------------------------------------------------------------------------------------
enum class Bucketing { kBlocks, kPartitionedRecords, kPartitionedOverlaps, kFixedSlots, kExactCsr };
// where duplicate removal runs: not at all (bounds as input), its two kernels on the main stream in front of everything,
// on the side stream beside the bucketing, its first pass inside the bucketing's counting pass (the side stream is left with
// the marked runs), its two kernels on the side stream beside the pile kernels
enum class DedupeAt { kNone, kMainInFront, kSideBesideBucketing, kInCountingPass, kSideBesidePiles };
// RALA_HIP_MEM_HOST_ASYNC columns: none on its way; each awaited by the kernel that reads it first; all of them awaited by
// the main and the side stream in front of the first kernel that reads one
enum class Columns { kOnDevice, kAsTheyCome, kAllAwaited };

struct InitPlan {
    Inputs input;
    Bucketing bucketing;
    uint32_t ev_shift;          // the CSR's offsets count units of 1 << ev_shift events
    DedupeAt dedupe;
    Columns columns;
    BucketTuning bt;            // (one look: what sizes the buffers fills them)
    bool fixed() const { return bucketing == Bucketing::kFixedSlots; }
    // duplicate removal on the side stream: the main stream joins it behind the pile kernels
    bool forked() const { return dedupe != DedupeAt::kNone && dedupe != DedupeAt::kMainInFront; }
};

// The plan from the context's options and sizes; exact_buckets: an earlier attempt of the call found a read with more events
// than a fixed slot holds (as the option use_fixed_buckets = 0).  Enqueues nothing.
int plan_initialize(rala_hip_ctx* ctx, bool exact_buckets, InitPlan& plan) {
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    if (ctx->rowless && ctx->debug_pile_stop_after != 99) {
        return fail(ctx, RALA_HIP_EINVAL, "debug_pile_stop_after is a diagnostic of the kernels that store rows: not with pile_rows = 0");
    }
    plan.input = !ctx->tuple_mode ? Inputs::kOverlaps : ctx->blocks_mode ? Inputs::kBlocks : ctx->records != nullptr ? Inputs::kRecords : Inputs::kTuples;
    plan.bt = {ctx->debug_part_shift, ctx->debug_count_window};
    // bucket bounds by read.  Fast path: one kernel into fixed slots of kRunEventCapBig events per
    // read (8 KB; 8 GB at a million reads - HBM is 288 GB); the position inside the slot is what the
    // counting atomic returns, so there is no scan and no second pass over the overlaps.  A read
    // with more events than a slot (only the position-space kernel could take it) sends the whole
    // data set through the exact CSR path.
    // Partitioned path (bucket_kernels.hip): the target side through two partitioning passes instead of one
    // memory-side atomic and one partial write per overlap; ends in the exact CSR.  Needs the overlaps
    // (not tuples), coordinates below 2^25, enough overlaps per partition for the passes to pay, few enough
    // reads for a histogram of their groups of 128 to fit the LDS (4.9 M).
    // (round 6: whichever pile kernel follows - the position-space kernel reads the rows' offsets in pairs as well)
    const bool fixed_allowed = ctx->use_fixed_buckets && !exact_buckets;
    const bool partition_allowed = fixed_allowed && ctx->use_partitioned_buckets;
    if (plan.input == Inputs::kBlocks) {
        // (an owner rank's blocks, scattered by partition on the senders: the partitioned path from level 2 on - there is no
        // other form of that input)
        plan.bucketing = Bucketing::kBlocks;
    } else if (plan.input == Inputs::kRecords && partition_allowed && partition_path_fits_records(n_reads, ctx->max_read_len, ctx->n_records, plan.bt)) {
        // (an owner rank's bound records: the same path from level 1 on, both sides as records; input that does not suit it
        // is turned into tuples)
        plan.bucketing = Bucketing::kPartitionedRecords;
    } else if (plan.input == Inputs::kOverlaps && partition_allowed && partition_path_fits(n_reads, ctx->max_read_len, ctx->n_ovl, plan.bt)) {
        plan.bucketing = Bucketing::kPartitionedOverlaps;
    } else if (ctx->use_run_kernel && fixed_allowed && (uint64_t)n_reads * kRunEventCapBig * 4ull <= (64ull << 30)) {
        plan.bucketing = Bucketing::kFixedSlots;
    } else {
        plan.bucketing = Bucketing::kExactCsr;
    }
    const bool partitioned = plan.bucketing == Bucketing::kBlocks || plan.bucketing == Bucketing::kPartitionedRecords ||
                             plan.bucketing == Bucketing::kPartitionedOverlaps;
    if (!partitioned && plan.input == Inputs::kOverlaps && ctx->n_ovl >= 0xFFFFFFF0ull / 4) {
        return fail(ctx, RALA_HIP_ETOOLARGE, "2^30 overlaps and more need the partitioned bucketing (its offsets count bound pairs); this input or these options rule it out");
    }
    // (the partitioned bucketing's offsets count bound pairs; option debug_ev_events = 1, tests and measurements: events where they fit)
    const uint64_t n_bounds = plan.bucketing == Bucketing::kBlocks ? ctx->n_block_records
                              : plan.bucketing == Bucketing::kPartitionedRecords ? ctx->n_records : 2 * ctx->n_ovl;
    plan.ev_shift = !partitioned || (ctx->debug_ev_events && 2 * n_bounds < 0xFFFFFFF0ull) ? 0u : kBucketPairShift;
    // duplicate removal only feeds the second pass (every resolvable overlap adds its bounds,
    // valid or not): it runs on a second stream and the main stream joins it after the pile kernels.
    // Beside WHAT it runs: beside the single-pass bucketing, both reading the same columns while the
    // atomics queue, the two slowed each other (0.2 - 0.5 ms per C3 step), so it starts when that
    // bucketing is done, beside the pile kernels.  Those are bound by instruction issue, and what runs
    // beside them costs them its whole stand-alone time (0.26 ms at C3: pile kernel 4.63 ms with it,
    // 4.37 without); the partitioned bucketing streams and has issue slots to spare - beside it the
    // duplicate removal costs 0.14 ms (round 4, docs/history/gpurun/r4_dedupe_early.sh: step 8.08 -> 7.99 ms).
    if (plan.input != Inputs::kOverlaps) {
        plan.dedupe = DedupeAt::kNone;
    } else if (!ctx->use_side_stream) {
        plan.dedupe = DedupeAt::kMainInFront;
    } else if (plan.bucketing != Bucketing::kPartitionedOverlaps) {
        plan.dedupe = DedupeAt::kSideBesidePiles;
    } else if (bucket_count_can_dedupe(ctx->ovl, ctx->d_valid.p)) {
        // (round 5) ... and inside the bucketing's counting pass where that pass can take it: both read the two id columns of every
        // overlap, the second stream is left with the marked queries' overlaps - usually none
        plan.dedupe = DedupeAt::kInCountingPass;
    } else {
        plan.dedupe = DedupeAt::kSideBesideBucketing;
    }
    // (columns on their way: only the path that names what it reads when takes them as they come)
    plan.columns = !ctx->upload_pending ? Columns::kOnDevice : plan.dedupe == DedupeAt::kInCountingPass ? Columns::kAsTheyCome : Columns::kAllAwaited;
    return RALA_HIP_OK;
}

// ---- the steps ----------------------------------------------------------------------------------------------------------------
// the rows' buffer (none with pile_rows = 0)
int place_rows(rala_hip_ctx* ctx) {
    if (ctx->rowless) {
        // option pile_rows = 0: no row is resident (what an earlier call allocated is given back); the kernels below store none
        ctx->d_pile.release();
        return RALA_HIP_OK;
    }
    // The rows as physical chunks of 1 GB mapped side by side into one range (round 6).  Where the rows lie physically decides
    // whether the first pile kernel takes 3.8 or 4.3 ms at C3 (five placements inside one process: 3.84 / 4.20 / 4.12 / 4.27 /
    // 3.81) - its stores, a wavefront per row, 7 000 rows open at a time, are the only access pattern of the path that feels it.
    // hipMalloc's single block landed anywhere in that range; chunks of 1 GB mapped in order: 3.73 - 3.86 in 25 placements of 25,
    // the bench line 7.19 - 7.22 ms in five processes against 7.36 - 7.55 alternating with them.
    // Option pile_chunk_mb (0 = one hipMalloc).  Falls back to hipMalloc where the driver refuses the mapping calls.
    hipError_t ec = hipErrorNotSupported;
    if (ctx->pile_chunk_mb > 0 && (ctx->pile_elems + 8) * sizeof(uint16_t) >= ((size_t)ctx->pile_chunk_mb << 20)) {
        ec = ctx->d_pile.ensure_chunked(ctx->pile_elems + 8, (size_t)ctx->pile_chunk_mb << 20, ctx->device, ctx->debug_chunk_fail);
        if (ec != hipSuccess) (void)hipGetLastError();
    }
    if (ec != hipSuccess) HIPCHECK(ctx->d_pile.ensure(ctx->pile_elems + 8));
    return RALA_HIP_OK;
}

// RALA_HIP_MEM_HOST_ASYNC: the columns leave the host now, in the order the kernels want them; a kernel waits for
// the event of the column it reads first (the copy stream is in order: a later event covers the earlier columns)
int queue_upload(rala_hip_ctx* ctx) {
    const size_t n4 = (size_t)ctx->n_ovl * 4;
    auto up = [&](int k) { return hipMemcpyAsync(ctx->d_ovl_u32[k].p, ctx->up_src[k], n4, hipMemcpyHostToDevice, ctx->copy); };
    // (a failed call may have left kernels that still read the columns: the copies behind them)
    HIPCHECK(hipStreamWaitEvent(ctx->copy, ctx->ev[kEvInitBegin], 0));
    HIPCHECK(up(0)); HIPCHECK(up(1));
    HIPCHECK(hipEventRecord(ctx->ev_up[0], ctx->copy));
    HIPCHECK(up(4)); HIPCHECK(up(5));
    HIPCHECK(hipEventRecord(ctx->ev_up[1], ctx->copy));
    HIPCHECK(up(2)); HIPCHECK(up(3));
    HIPCHECK(hipEventRecord(ctx->ev_up[2], ctx->copy));
    HIPCHECK(up(6));
    HIPCHECK(hipMemcpyAsync(ctx->d_ovl_strand.p, ctx->up_strand, ctx->n_ovl, hipMemcpyHostToDevice, ctx->copy));
    HIPCHECK(hipEventRecord(ctx->ev_up[3], ctx->copy));      // everything
    ctx->upload_queued = true;
    return RALA_HIP_OK;
}

int wait_for_all_columns(rala_hip_ctx* ctx) {
    HIPCHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_up[3], 0));
    HIPCHECK(hipStreamWaitEvent(ctx->side, ctx->ev_up[3], 0));
    return RALA_HIP_OK;
}

// Duplicate removal on stream st, kEvInitDedupeDone behind it: its own two kernels, or - fix, where the bucketing's counting
// pass has marked the runs that need the full comparison - the kernel over those.  On the side stream it starts behind the
// event `behind` (none on the main stream: -1) and, where columns are still on their way, behind `columns` (the last of them).
int queue_dedupe(rala_hip_ctx* ctx, hipStream_t st, int behind, const BucketDedupe* fix = nullptr, hipEvent_t columns = nullptr) {
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    if (behind >= 0) HIPCHECK(hipStreamWaitEvent(st, ctx->ev[behind], 0));
    if (columns) HIPCHECK(hipStreamWaitEvent(st, columns, 0));
    if (fix) launch_dedupe_fix(ctx->ovl, n_reads, *fix, st);
    else launch_dedupe(ctx->ovl, n_reads, ctx->d_suspect.p, ctx->d_valid.p, st);
    HIPCHECK(hipEventRecord(ctx->ev[kEvInitDedupeDone], st));
    return RALA_HIP_OK;
}

int bucket_from_blocks(rala_hip_ctx* ctx, const InitPlan& plan, FillList& fills) {
    const ShardGeometry& g = ctx->shard_geom;
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    HIPCHECK(ctx->d_shard_group.ensure(shard_group_words(g)));
    HIPCHECK(ctx->d_shard_tiles.ensure(3 * shard_tile_slots(g, ctx->n_block_records) + 2));
    HIPCHECK(ctx->d_bk_rec[1].ensure((size_t)ctx->n_block_records + 64));
    HIPCHECK(launch_bucket_from_blocks(ctx->blocks_base, ctx->blocks_base_self, ctx->blocks, g, n_reads, ctx->n_block_records,
                                       ctx->d_shard_group.p, ctx->d_shard_tiles.p, ctx->d_bk_rec[1].p, ctx->d_ev_off.p, ctx->d_ev.p, fills, ctx->stream, plan.ev_shift));
    return RALA_HIP_OK;
}

// the partitioned path over bound records or over the overlaps - over those with duplicate removal inside the counting pass
// where the plan says so
int bucket_partitioned(rala_hip_ctx* ctx, const InitPlan& plan, FillList& fills) {
    hipStream_t s = ctx->stream;
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    const bool from_records = plan.bucketing == Bucketing::kPartitionedRecords;
    const BucketTuning& bt = plan.bt;
    const uint64_t n_rec = from_records ? ctx->n_records : ctx->n_ovl;
    for (int k = 0; k < 3; ++k) HIPCHECK(ctx->d_bk_u32[k].ensure(n_reads + 2));
    HIPCHECK(ctx->d_bk_part.ensure(partition_count(n_reads, bt) + 2));
    HIPCHECK(ctx->d_bk_group.ensure(3 * (size_t)partition_group_slots(n_reads, bt)));
    HIPCHECK(ctx->d_bk_tiles.ensure(3 * partition_tile_slots(n_reads, n_rec, bt) + 2));
    for (int k = 0; k < 2; ++k) HIPCHECK(ctx->d_bk_rec[k].ensure(partition_records_needed(n_reads, n_rec)));
    if (from_records) {
        HIPCHECK(launch_bucket_partitioned_records(ctx->records, ctx->n_records, n_reads, bt, ctx->d_bk_u32[0].p, ctx->d_bk_part.p,
                                                   ctx->d_bk_group.p, ctx->d_bk_tiles.p, ctx->d_bk_rec[0].p, ctx->d_bk_rec[1].p,
                                                   ctx->d_ev_off.p, ctx->d_ev.p, ctx->n_compute_units, fills, s, 15u, plan.ev_shift));
        return RALA_HIP_OK;
    }
    const bool counted = plan.dedupe == DedupeAt::kInCountingPass;
    BucketDedupe bd = {};
    if (counted) {
        // (the marks' count: zeroed with d_small by the call's fill)
        const int rc = counted_dedupe(ctx, ctx->d_small.p + kInitDedupeMarks, ctx->ev[kEvBucketCounted], bd);
        if (rc != RALA_HIP_OK) return rc;
        if (plan.columns == Columns::kAsTheyCome) { bd.ids = ctx->ev_up[0]; bd.b_coords = ctx->ev_up[1]; bd.a_coords = ctx->ev_up[2]; }
    }
    HIPCHECK(launch_bucket_partitioned(ctx->ovl, n_reads, bt, ctx->d_bk_u32[0].p, ctx->d_bk_u32[2].p,
                                       ctx->d_bk_part.p, ctx->d_bk_group.p, ctx->d_bk_tiles.p, ctx->d_bk_rec[0].p,
                                       ctx->d_bk_rec[1].p, ctx->d_ev_off.p, ctx->d_ev.p, ctx->n_compute_units, fills, s,
                                       counted ? &bd : nullptr, plan.ev_shift));
    if (!counted) return RALA_HIP_OK;
    // (the side stream is left with the marked runs; of columns on their way it still needs the lengths)
    return queue_dedupe(ctx, ctx->side, kEvBucketCounted, &bd, plan.columns == Columns::kAsTheyCome ? ctx->ev_up[3] : nullptr);
}

int bucket_fixed_slots(rala_hip_ctx* ctx, FillList& fills) {
    hipStream_t s = ctx->stream;
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    const uint32_t slot = kRunEventCapBig;          // (pile_args' stride)
    HIPCHECK(ctx->d_ev_fixed.ensure((size_t)n_reads * slot + 8));
    HIPCHECK(ctx->d_cc_flags.ensure(kCcFlagsWords));
    fills.add(ctx->d_cursor.p, 0, (size_t)(n_reads + 1) * 4);
    HIPCHECK(fills.launch(s));
    // (the slot-overflow flag and the count of dead reads live in d_small, zeroed by the call's fill and
    // fetched in one copy with the other results)
    if (ctx->tuple_mode) {
        launch_bucket_fixed_tuples(ctx->tuples, ctx->n_tuples, n_reads, slot, ctx->d_cursor.p,
                                   ctx->d_ev_fixed.p, ctx->d_small.p + kInitSlotOverflow, s);
    } else {
        launch_bucket_fixed(ctx->ovl, n_reads, slot, ctx->d_cursor.p, ctx->d_ev_fixed.p, ctx->d_small.p + kInitSlotOverflow, s);
    }
    // the overflow flag is read together with the other results at the end of the attempt; a
    // set flag repeats it on the exact path (no host round trip in the common case)
    return RALA_HIP_OK;
}

// count -> exclusive scan -> scatter
int bucket_exact_csr(rala_hip_ctx* ctx, FillList& fills) {
    hipStream_t s = ctx->stream;
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    fills.add(ctx->d_cursor.p, 0, (size_t)(n_reads + 1) * 4);
    HIPCHECK(fills.launch(s));
    if (ctx->tuple_mode) {
        launch_count_tuples(ctx->tuples, ctx->n_tuples, n_reads, ctx->d_cursor.p, s);
    } else {
        HIPCHECK(ctx->d_slot_rank[0].ensure(ctx->n_ovl + 1)); HIPCHECK(ctx->d_slot_rank[1].ensure(ctx->n_ovl + 1));
        launch_count_bounds(ctx->ovl, n_reads, ctx->d_cursor.p, ctx->d_slot_rank[0].p, ctx->d_slot_rank[1].p, s);
    }
    launch_exclusive_scan(ctx->d_cursor.p, ctx->d_ev_off.p, n_reads, ctx->d_scan_ws.p, s);
    if (ctx->tuple_mode) {
        HIPCHECK(hipMemcpyAsync(ctx->d_cursor.p, ctx->d_ev_off.p, (size_t)n_reads * 4, hipMemcpyDeviceToDevice, s));
        launch_scatter_tuples(ctx->tuples, ctx->n_tuples, n_reads, ctx->d_cursor.p, ctx->d_ev.p, s);
    } else {
        launch_scatter_bounds(ctx->ovl, n_reads, ctx->d_ev_off.p, ctx->d_slot_rank[0].p, ctx->d_slot_rank[1].p, ctx->d_ev.p, s);
    }
    return RALA_HIP_OK;
}

// the bound events by read, on the plan's path; fills: what the call wants cleared, launched with the path's own clears
int bucket(rala_hip_ctx* ctx, const InitPlan& plan, FillList& fills) {
    if (plan.input == Inputs::kRecords && plan.bucketing != Bucketing::kPartitionedRecords) {
        HIPCHECK(ctx->d_tuple.ensure(2 * ctx->n_records + 8));
        launch_records_to_tuples(ctx->records, ctx->n_records, ctx->d_tuple.p, ctx->stream);
        ctx->tuples = ctx->d_tuple.p;
        ctx->n_tuples = 2 * ctx->n_records;
    }
    switch (plan.bucketing) {
    case Bucketing::kBlocks: return bucket_from_blocks(ctx, plan, fills);
    case Bucketing::kPartitionedRecords:
    case Bucketing::kPartitionedOverlaps: return bucket_partitioned(ctx, plan, fills);
    case Bucketing::kFixedSlots: return bucket_fixed_slots(ctx, fills);
    case Bucketing::kExactCsr: break;
    }
    return bucket_exact_csr(ctx, fills);
}

// the pile kernels' arguments for this attempt
int first_pass_args(rala_hip_ctx* ctx, const InitPlan& plan, PileArgs& a) {
    a = pile_args(ctx, primary_events(ctx, plan.fixed(), plan.ev_shift));
    a.rows_chunked = ctx->d_pile.reserved ? 1u : 0u;
    a.slab = ctx->d_slab.p;
    a.stop_after = (uint32_t)ctx->debug_pile_stop_after;
    a.alive = ctx->d_alive.p; a.n_pits = ctx->d_n_pits.p; a.n_hills = ctx->d_n_hills.p; a.iv_slot = ctx->d_iv_slot.p;
    a.pool = ctx->d_pool.p; a.pool_count = ctx->d_small.p + kInitPoolCount; a.pool_cap = ctx->pool_cap;
    a.error = ctx->d_small.p + kInitStatus;
    // (what outgrows the position-space kernel's LDS lists: noted, and dealt with after the attempt's one look from the host)
    HIPCHECK(ctx->d_big_list[0].ensure((uint32_t)ctx->n_reads + 1));
    a.big_list = ctx->d_big_list[0].p; a.big_count = ctx->d_small.p + kInitNotedReads;
    a.force_big = ctx->debug_force_big ? 1u : 0u;
    return RALA_HIP_OK;
}

// Chain without host synchronisation.  Every read starts in the kernel that fits it, known
// beforehand: by length class (set_reads sorted them) and by event count (listed from the
// bucket counts).  A hand-over through a list behind the first kernel costs one atomic on
// one counter per read (1 ms for 100 000 reads) and puts the small, latency-bound kernels
// behind the big one (0.2 ms per C3 step); now they run beside it on a stream of their own:
//   main  up to 16384 bases, up to 512 events: run-space kernel, seven wavefronts per SIMD,
//         one workgroup per read
//   aux   more than 512 events (dense list) -> cap 1024;  up to 32768 bases -> the short
//         layout with a bitmap twice the size (four wavefronts per SIMD, 9 % faster on
//         20 kb reads than what follows);  longer -> cap 512 for any length (sorted events)
// What still does not fit its kernel (slope-region lists, event caps) goes to a list: of
// the cap-512 kernels (list 1) -> cap 1024, of those (list 2) -> cap 2048 -> what is left
// (list 3) to the position-space kernel, sized for the longest read.  These run on the
// main stream behind the join, usually over nothing.
// (a: left as the last kernel took it - the noted reads run with it)
int run_pile_chain(rala_hip_ctx* ctx, PileArgs& a) {
    hipStream_t s = ctx->stream;
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    HIPCHECK(ctx->d_overflow_mid.ensure(n_reads + 1));
    HIPCHECK(ctx->d_dense.ensure(n_reads + 1));
    uint32_t* list_dense = ctx->d_dense.p;
    uint32_t* list1 = ctx->d_overflow.p;
    uint32_t* list2 = ctx->d_overflow_mid.p;
    uint32_t* list3 = ctx->d_order.p;
    // (all four zeroed with d_small by the call's fill)
    uint32_t* cnt_dense = ctx->d_small.p + kInitDenseReads;
    uint32_t* cnt1 = ctx->d_small.p + kInitToCap1024;
    uint32_t* cnt2 = ctx->d_small.p + kInitToCap2048;
    uint32_t* cnt3 = ctx->d_small.p + kInitToPosition;
    const uint32_t n_short = ctx->n_class[0], n_medium = ctx->n_class[1], n_long = ctx->n_class[2];
    const uint32_t* by_class = n_short != n_reads ? ctx->d_class_order.p : nullptr;
    // few longer reads: the first kernel goes over all reads without the indirection (2 % at C3)
    // and leaves at once for a longer one
    const bool short_by_list = by_class && (uint64_t)(n_reads - n_short) * 8 > n_reads;
    hipStream_t aux = ctx->use_side_stream ? ctx->aux : s;
    if (aux != s) HIPCHECK(hipStreamWaitEvent(aux, ctx->ev[kEvInitBucketed], 0));
    a.lw = 0;
    a.skip_dense = 1;
    launch_pile_dense_list(a, n_reads, list_dense, cnt_dense, aux);
    a.order = list_dense;
    a.n_items = n_reads;
    a.n_items_dev = cnt_dense;
    launch_pile_runs(a, std::min<uint32_t>(n_reads, 8192), PileTier::kCap1024, list2, cnt2, aux);
    a.n_items_dev = nullptr;
    a.order = by_class ? by_class + n_short : nullptr;
    a.n_items = n_medium;
    launch_pile_runs(a, std::min<uint32_t>(n_medium, 16384), PileTier::kUpTo32k, list1, cnt1, aux);
    a.order = by_class ? by_class + n_short + n_medium : nullptr;
    a.n_items = n_long;
    launch_pile_runs(a, std::min<uint32_t>(n_long, 20480), PileTier::kAnyLength, list1, cnt1, aux);
    if (aux != s) HIPCHECK(hipEventRecord(ctx->ev[kEvPileAuxDone], aux));
    a.order = short_by_list ? by_class : nullptr;
    a.n_items = short_by_list ? n_short : n_reads;
    launch_pile_runs(a, a.n_items, PileTier::kCap512First, list1, cnt1, s);
    if (aux != s) HIPCHECK(hipStreamWaitEvent(s, ctx->ev[kEvPileAuxDone], 0));
    a.n_items = n_reads;
    a.order = list1;
    a.n_items_dev = cnt1;
    launch_pile_runs(a, std::min<uint32_t>(n_reads, 8192), PileTier::kCap1024, list2, cnt2, s);
    a.order = list2;
    a.n_items_dev = cnt2;
    launch_pile_runs(a, std::min<uint32_t>(n_reads, 2048), PileTier::kCap2048, list3, cnt3, s);
    a.order = list3;
    a.n_items_dev = cnt3;
    const uint32_t max_len = ctx->max_read_len;
    const bool in_lds = (int64_t)max_len <= ctx->max_lds_read_len && pile_lw_for(max_len) <= 24576;
    a.lw = pile_lw_for(max_len);
    const uint32_t grid = std::min<uint32_t>(n_reads, 256);
    if (!in_lds) HIPCHECK(ctx->d_slab.ensure((size_t)grid * 3 * a.lw));
    a.slab = ctx->d_slab.p;
    launch_pile_build_annotate(a, grid, in_lds, s);
    ctx->tm.pile_launches = 5 + (n_medium ? 1 : 0) + (n_long ? 1 : 0);
    return RALA_HIP_OK;
}

// The attempt's one look from the host: the words of d_small, with the count of dead reads; the reads that outgrew the
// position-space kernel's LDS lists run again behind it (not where a slot overflowed: that attempt's results are dropped).
// From here on the host's columns are the caller's again.
int look_at_results(rala_hip_ctx* ctx, const InitPlan& plan, const PileArgs& a, uint32_t (&small)[kSmallWords]) {
    hipStream_t s = ctx->stream;
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    // the per-read results stay on the device; host mirrors are fetched by the first getter
    launch_count_zero_u8(ctx->d_alive.p, n_reads, ctx->d_small.p + kInitDeadReads, s);
    HIPCHECK(d2h_small(ctx, small, ctx->d_small.p, sizeof(small), s));
    HIPCHECK(stream_sync(ctx, s));
    if (plan.columns != Columns::kOnDevice) {
        // (the host's columns are free from here on)
        HIPCHECK(hipStreamSynchronize(ctx->copy));
        upload_done(ctx);
    }
    const uint32_t slot_overflow = plan.fixed() ? small[kInitSlotOverflow] : 0;
    if (small[kInitNotedReads] && !slot_overflow) {
        // reads whose region / interval lists outgrew the position-space kernel's LDS lists
        const int rc_big = run_unbounded_piles(ctx, a, small[kInitNotedReads], ctx->d_small.p + kInitNotedReads);
        if (rc_big != RALA_HIP_OK) return rc_big;
        HIPCHECK(hipMemsetAsync(ctx->d_small.p + kInitDeadReads, 0, 4, s));
        launch_count_zero_u8(ctx->d_alive.p, n_reads, ctx->d_small.p + kInitDeadReads, s);
        const uint32_t noted = small[kInitNotedReads];
        HIPCHECK(d2h_small(ctx, small, ctx->d_small.p, sizeof(small), s));
        HIPCHECK(stream_sync(ctx, s));
        small[kInitNotedReads] = noted;
    }
    return RALA_HIP_OK;
}

// what an attempt asks of the call when its results do not stand
struct Again {
    bool exact_buckets = false;     // some read has more events than a fixed slot holds: once more, through the exact path
    uint32_t pool = 0;              // more pits and hills than the interval pool holds: once more, with a pool of this size
    bool wanted() const { return exact_buckets || pool != 0; }
};

// the counters and times of the attempt into ctx->tm, its errors, what it asks for (again), the context's new state
int settle(rala_hip_ctx* ctx, const InitPlan& plan, const uint32_t (&small)[kSmallWords], Again& again) {
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    if (plan.fixed() && small[kInitSlotOverflow]) {
        again.exact_buckets = true;
        return RALA_HIP_OK;
    }
    const uint32_t n_dead = small[kInitDeadReads];
    ctx->tm.pile_overflow_reads = ctx->use_run_kernel ? small[kInitDenseReads] + small[kInitToCap1024] : 0;      // event-dense + handed on
    if (trace_on() || getenv("RALA_HIP_TRACE_BUFFERS")) {
        fprintf(stderr, "[trace] buffers: events %p (CSR %p) slots %p counts %p piles %p a_id %p b_id %p b_begin %p\n", (void*)ctx->d_ev.p, (void*)ctx->d_ev_off.p, (void*)ctx->d_ev_fixed.p,
                (void*)ctx->d_cursor.p, (void*)ctx->d_pile.p, (const void*)ctx->ovl.a_id, (const void*)ctx->ovl.b_id,
                (const void*)ctx->ovl.b_begin);
        if (trace_on()) fprintf(stderr, "[trace] pile chain: %u reads listed as event-dense, %u handed on by the cap-512 kernels, %u on to cap 2048, %u to position space\n",
                small[kInitDenseReads], small[kInitToCap1024], small[kInitToCap2048], small[kInitToPosition]);
    }
    ctx->tm.pile_position_reads = ctx->use_run_kernel ? small[kInitToPosition] : n_reads;
    // dedupe_ms: what duplicate removal adds to the critical path (it runs beside the bucketing
    // and the pile kernels; the main stream joins it after them)
    {
        const bool forked = plan.forked();
        float dd = 0, bk = 0, all = 0;
        HIPCHECK(hipEventElapsedTime(&dd, ctx->ev[kEvInitBegin], ctx->ev[kEvInitDedupeDone]));
        HIPCHECK(hipEventElapsedTime(&bk, forked ? ctx->ev[kEvInitBegin] : ctx->ev[kEvInitDedupeDone], ctx->ev[kEvInitBucketed]));
        HIPCHECK(hipEventElapsedTime(&all, ctx->ev[kEvInitBegin], ctx->ev[kEvInitPilesDone]));
        ctx->tm.bucket_ms = bk;
        ctx->tm.dedupe_ms = forked ? std::max(0.0f, dd - all) : dd;
    }
    HIPCHECK(hipEventElapsedTime(&ctx->tm.pile_ms, ctx->ev[kEvInitBucketed], ctx->ev[kEvInitPilesDone]));
    if (small[kInitStatus] & (kErrRegionCapacity | kErrRawCapacity)) return fail(ctx, RALA_HIP_EDEVICE, "slope-region list overflow in the pile kernel");
    if (small[kInitStatus] & kErrPoolCapacity) {
        // more pits and hills than the pool holds (interval_pool_per_read_x1000 is a hint): its counter holds what is needed -
        // once more with a pool of that size (and a little more: the slots of reads that ran twice are not handed back)
        again.pool = grown_pool_size(small[kInitPoolCount], ctx->pool_cap);
        if (!again.pool) return fail(ctx, RALA_HIP_ENOMEM, "interval pool beyond 2^32 entries");
        return RALA_HIP_OK;
    }
    state_installed(ctx, n_dead, std::min(small[kInitPoolCount], ctx->pool_cap), true, plan.fixed(), !ctx->tuple_mode);
    if (ctx->n_prefiltered == ctx->n_reads) return fail(ctx, RALA_HIP_EFILTERED, "filtered all sequences");
    return RALA_HIP_OK;
}

// One attempt of rala_hip_initialize: the plan, its steps, the look.  Returns RALA_HIP_OK with `again` set where the call
// has to run it once more.
int initialize_attempt(rala_hip_ctx* ctx, bool exact_buckets, Again& again) {
    if (ctx->n_reads == 0) return fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (!ctx->inputs_set) return fail(ctx, RALA_HIP_EINVAL, "no overlaps or bound tuples set");
    HIPCHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    ctx->tm = rala_hip_timings();
    ctx->overlaps.clear(); ctx->internals.clear();
    initialize_begun(ctx);
    ctx->rows_materialised = 0;
    InitPlan plan;
    int rc = plan_initialize(ctx, exact_buckets, plan);
    if (rc != RALA_HIP_OK) return rc;
    rc = place_rows(ctx);
    if (rc != RALA_HIP_OK) return rc;
    // (whatever a failed call may have left on the aux stream ends before the counters are reset)
    HIPCHECK(hipEventRecord(ctx->ev[kEvAuxDrained], ctx->aux));
    HIPCHECK(hipStreamWaitEvent(s, ctx->ev[kEvAuxDrained], 0));
    HIPCHECK(hipEventRecord(ctx->ev[kEvInitBegin], s));
    if (plan.columns != Columns::kOnDevice) {
        rc = queue_upload(ctx);
        if (rc != RALA_HIP_OK) return rc;
    }
    // the call's counters and what the bucketing wants cleared: one fill (fill_kernels.hip)
    FillList fills;
    fills.add(ctx->d_small.p, 0, kSmallWords * 4);
    if (plan.columns == Columns::kAllAwaited) {
        rc = wait_for_all_columns(ctx);
        if (rc != RALA_HIP_OK) return rc;
    }
    switch (plan.dedupe) {
    case DedupeAt::kNone: HIPCHECK(hipEventRecord(ctx->ev[kEvInitDedupeDone], s)); break;        // (the timings read the event)
    case DedupeAt::kMainInFront: rc = queue_dedupe(ctx, s, -1); break;
    case DedupeAt::kSideBesideBucketing: rc = queue_dedupe(ctx, ctx->side, kEvInitBegin); break;
    case DedupeAt::kInCountingPass:             // (in bucket_partitioned)
    case DedupeAt::kSideBesidePiles: break;     // (behind the bucketing, below)
    }
    if (rc != RALA_HIP_OK) return rc;
    rc = bucket(ctx, plan, fills);
    if (rc != RALA_HIP_OK) return rc;
    HIPCHECK(hipEventRecord(ctx->ev[kEvInitBucketed], s));
    if (plan.dedupe == DedupeAt::kSideBesidePiles) {
        rc = queue_dedupe(ctx, ctx->side, kEvInitBucketed);
        if (rc != RALA_HIP_OK) return rc;
    }

    ctx->ev_shift = plan.ev_shift;
    PileArgs a;
    rc = first_pass_args(ctx, plan, a);
    if (rc != RALA_HIP_OK) return rc;
    if (ctx->use_run_kernel) {
        rc = run_pile_chain(ctx, a);
    } else {
        std::vector<uint32_t> reads(ctx->n_reads);
        std::iota(reads.begin(), reads.end(), 0u);
        rc = run_position_kernel(ctx, a, reads);
    }
    if (rc != RALA_HIP_OK) return rc;
    HIPCHECK(hipEventRecord(ctx->ev[kEvInitPilesDone], s));
    HIPCHECK(hipGetLastError());
    if (plan.forked()) HIPCHECK(hipStreamWaitEvent(s, ctx->ev[kEvInitDedupeDone], 0));

    uint32_t small[kSmallWords];
    rc = look_at_results(ctx, plan, a, small);
    if (rc != RALA_HIP_OK) return rc;
    return settle(ctx, plan, small, again);
}

// The attempts of one call.  What an attempt asked for holds for the later ones; tm is the last attempt's, its pool_regrown
// the call's.
int initialize_until_it_fits(rala_hip_ctx* ctx) {
    bool exact_buckets = false;
    uint32_t regrown = 0;
    for (;;) {
        Again again;
        const int rc = initialize_attempt(ctx, exact_buckets, again);
        if (regrown) ctx->tm.pool_regrown = regrown;       // (tm: reset by the attempt that followed the regrow)
        if (rc != RALA_HIP_OK || !again.wanted()) return rc;
        if (again.exact_buckets) exact_buckets = true;
        if (again.pool) {
            ctx->pool_cap = again.pool;
            HIPCHECK(ctx->d_pool.ensure(ctx->pool_cap));
            ++regrown;
        }
    }
}

int emit_bucketed(rala_hip_ctx* ctx, uint32_t world, uint64_t* tuples_dev, uint64_t* counts, bool records) {
    if (!ctx || !tuples_dev || !counts || world == 0 || world > 64) return RALA_HIP_EINVAL;
    if (((uintptr_t)tuples_dev & 15u) != 0) return fail(ctx, RALA_HIP_EINVAL, "tuple buffer must be 16-byte aligned");
    HIPCHECK(hipSetDevice(ctx->device));
    { const int rcu = flush_upload(ctx); if (rcu != RALA_HIP_OK) return rcu; }
    hipStream_t s = ctx->stream;
    HIPCHECK(ctx->d_owner_cnt.ensure(2 * 64));
    uint32_t* cnt = ctx->d_owner_cnt.p;
    uint32_t* cur = cnt + 64;
    HIPCHECK(hipMemsetAsync(cnt, 0, 2 * 64 * 4, s));
    launch_bucket_tuples(ctx->ovl, (uint32_t)ctx->n_reads, world, 0, cnt, (uint2*)tuples_dev, s, records);
    // (the buckets' places from the counts on the device: the host looks once, at the end)
    launch_owner_offsets(cnt, world, cur, s);
    launch_bucket_tuples(ctx->ovl, (uint32_t)ctx->n_reads, world, 1, cur, (uint2*)tuples_dev, s, records);
    uint32_t h[64];
    HIPCHECK(d2h_small(ctx, h, cnt, world * 4, s));
    HIPCHECK(stream_sync(ctx, s));
    HIPCHECK(hipGetLastError());
    for (uint32_t p = 0; p < world; ++p) counts[p] = h[p];
    return RALA_HIP_OK;
}

}  // namespace

// A sender of a sharded run: duplicate removal on the side stream (joined by the second pass), the bounds of the slice
// scattered once by (owner, partition) into `send` (shard_send_words() words); words[p] = 8-byte words of owner p's block.
int rala_hip::shard_emit(rala_hip_ctx* ctx, const ShardGeometry& g, uint64_t* send, uint64_t* words) {
    if (!ctx || !send || !words) return RALA_HIP_EINVAL;
    if (ctx->n_reads == 0) return fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (!ctx->inputs_set || ctx->tuple_mode) return fail(ctx, RALA_HIP_EINVAL, "no overlaps set");
    HIPCHECK(hipSetDevice(ctx->device));
    { const int rcu = flush_upload(ctx); if (rcu != RALA_HIP_OK) return rcu; }
    hipStream_t s = ctx->stream;
    const uint32_t n_reads = (uint32_t)ctx->n_reads;
    // duplicate removal: its first pass inside the count where that kernel can take it (the id columns on 16-byte boundaries),
    // the marked runs' fix on the side stream beside the scatter - as on one GPU (rala_hip_initialize); otherwise the two
    // kernels of its own beside the whole emit
    const bool counted = ctx->use_side_stream && bucket_count_can_dedupe(ctx->ovl, ctx->d_valid.p);
    BucketDedupe bd = {};
    if (counted) {
        // (the marks' count: the word behind the list)
        const int rcd = counted_dedupe(ctx, nullptr, ctx->ev[kEvEmitCounted], bd);
        if (rcd != RALA_HIP_OK) return rcd;
        HIPCHECK(hipMemsetAsync(bd.list_count, 0, 4, s));
    } else if (ctx->use_side_stream) {
        HIPCHECK(hipEventRecord(ctx->ev[kEvEmitCounted], s));
        HIPCHECK(hipStreamWaitEvent(ctx->side, ctx->ev[kEvEmitCounted], 0));
        launch_dedupe(ctx->ovl, n_reads, ctx->d_suspect.p, ctx->d_valid.p, ctx->side);
        HIPCHECK(hipEventRecord(ctx->ev[kEvEmitDedupeDone], ctx->side));
        dedupe_forked(ctx);
    } else {
        launch_dedupe(ctx->ovl, n_reads, ctx->d_suspect.p, ctx->d_valid.p, s);
    }
    validity_bits_ready(ctx);
    HIPCHECK(ctx->d_shard_group.ensure((size_t)g.world * g.groups + 2));
    HIPCHECK(ctx->d_shard_part.ensure((size_t)g.world * g.n_part + 2));
    HIPCHECK(ctx->d_shard_words.ensure(64));
    FillList fills;
    HIPCHECK(launch_shard_emit(ctx->ovl, n_reads, g, ctx->d_shard_group.p, ctx->d_shard_part.p, send, ctx->d_shard_words.p,
                               ctx->n_compute_units, fills, s, counted ? &bd : nullptr));
    if (counted && ctx->n_ovl) {
        HIPCHECK(hipStreamWaitEvent(ctx->side, ctx->ev[kEvEmitCounted], 0));
        launch_dedupe_fix(ctx->ovl, n_reads, bd, ctx->side);
        HIPCHECK(hipEventRecord(ctx->ev[kEvEmitDedupeDone], ctx->side));
        dedupe_forked(ctx);
    }
    uint32_t h[64];
    HIPCHECK(d2h_small(ctx, h, ctx->d_shard_words.p, g.world * 4, s));
    HIPCHECK(stream_sync(ctx, s));
    HIPCHECK(hipGetLastError());
    for (uint32_t p = 0; p < g.world; ++p) words[p] = h[p];
    return RALA_HIP_OK;
}

extern "C" {

int rala_hip_initialize(rala_hip_ctx* ctx) {
    if (!ctx) return RALA_HIP_EINVAL;
    const int rc = initialize_until_it_fits(ctx);
    // RALA_HIP_MEM_HOST_ASYNC: the host's columns are the caller's again when this call returns - however it returns
    // (only a first attempt finds columns on their way, and an attempt that asks for another has seen them arrive)
    if (ctx->upload_pending && ctx->copy) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->copy);
        // (a call that left before it had queued the copies has uploaded nothing: the next reader does, flush_upload)
        if (ctx->upload_queued) upload_done(ctx);
    }
    ctx->upload_queued = false;
    return rc;
}

int rala_hip_dedupe(rala_hip_ctx* ctx) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (ctx->n_reads == 0) return fail(ctx, RALA_HIP_EINVAL, "no reads set");
    if (!ctx->inputs_set || ctx->tuple_mode) return fail(ctx, RALA_HIP_EINVAL, "no overlaps set");
    HIPCHECK(hipSetDevice(ctx->device));
    { const int rcu = flush_upload(ctx); if (rcu != RALA_HIP_OK) return rcu; }
    launch_dedupe(ctx->ovl, (uint32_t)ctx->n_reads, ctx->d_suspect.p, ctx->d_valid.p, ctx->stream);
    HIPCHECK(stream_sync(ctx, ctx->stream));
    HIPCHECK(hipGetLastError());
    validity_bits_ready(ctx);
    return RALA_HIP_OK;
}

int rala_hip_emit_bound_tuples(rala_hip_ctx* ctx, uint64_t* tuples_dev) {
    if (!ctx || !tuples_dev) return RALA_HIP_EINVAL;
    if (((uintptr_t)tuples_dev & 15u) != 0) return fail(ctx, RALA_HIP_EINVAL, "tuple buffer must be 16-byte aligned");
    HIPCHECK(hipSetDevice(ctx->device));
    { const int rcu = flush_upload(ctx); if (rcu != RALA_HIP_OK) return rcu; }
    launch_emit_tuples(ctx->ovl, (uint32_t)ctx->n_reads, (uint2*)tuples_dev, ctx->stream);
    HIPCHECK(stream_sync(ctx, ctx->stream));
    HIPCHECK(hipGetLastError());
    return RALA_HIP_OK;
}

int rala_hip_emit_bound_tuples_bucketed(rala_hip_ctx* ctx, uint32_t world, uint64_t* tuples_dev, uint64_t* counts) {
    return emit_bucketed(ctx, world, tuples_dev, counts, false);
}
int rala_hip_bound_records_fit(const rala_hip_ctx* ctx, uint32_t world) {
    if (!ctx || world == 0) return 0;
    const uint64_t local = (ctx->n_reads + world - 1) / world;
    return ctx->max_read_len < (1u << kBoundRecordCoordBits) - 32u && local < (1ull << kBoundRecordReadBits) ? 1 : 0;
}
int rala_hip_emit_bound_records_bucketed(rala_hip_ctx* ctx, uint32_t world, uint64_t* records_dev, uint64_t* counts) {
    if (!ctx) return RALA_HIP_EINVAL;
    if (!rala_hip_bound_records_fit(ctx, world)) return fail(ctx, RALA_HIP_EINVAL, "reads too long or too many for bound records");
    return emit_bucketed(ctx, world, records_dev, counts, true);
}

}  // extern "C"
